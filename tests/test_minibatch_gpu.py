"""Minibatch PPO updates on the GPU (mhppo.ppo.train_minibatches, Algo_PPO(minibatches=K)): the
driver against a loop of train_epoch calls over Heads built from host-permuted, sliced copies of
the same buckets, bit for bit (the train kernels are deterministic in (rows, M), so equality is the
expectation: a difference is a finding to name, not a tolerance to add); the knob off; resume; the
step counts; K beyond a head's rows / 4; the constructor's checks.  coop 2/1/2 at 64 envs."""
import math

import numpy as np
import pytest
import torch

import shuffle_ref as sr

pytestmark = pytest.mark.gpu
NAMES = ("cross", "wait", "choice")


def _algo(seed=0, n_envs=64, **kw):
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    venv = VecCrosswalk("coop", n_envs, 2, 1, 2, seed_base=3)
    torch.manual_seed(seed)
    return Algo_PPO(Model_PPO, venv, verbose=False, save_curves=False, **kw)


def _rows_seen(a):
    """A list that receives, per iteration, the row count of each head's batch (train() clears the
    buckets at the end of an iteration)."""
    seen, upd = [], a.update

    def update():
        seen.append({n: getattr(a.rollout, n)["ret"].numel() for n in NAMES})
        return upd()

    a.update = update
    return seen


def _collect(a):
    a.rollout.reset()
    a.rollout.iterations_rand(a.actor_net_cross, a.actor_net_wait, a.actor_net_choice)
    return {n: {k: getattr(a.rollout, n)[k].clone() for k in ("obs", "act", "logp", "ret")} for n in NAMES}


def _heads(a, buckets, per_row, rows=None):
    """ppo.Heads of `a`'s nets over `buckets` (rows: per name an index tensor of the rows to keep);
    the choice head's counts are its rows' own."""
    from mhppo import ppo
    heads = []
    for name in NAMES:
        b = buckets[name]
        if rows is not None:
            b = {k: v[rows[name]] for k, v in b.items()}
        m = b["ret"].numel()
        if m == 0:
            heads.append(None)
            continue
        kind = "d" if name == "choice" else "c"
        counts = torch.stack([(b["act"] == 0).sum(), (b["act"] == 1).sum()]).double() if kind == "d" else None
        heads.append(ppo.Head(kind, getattr(a, f"actor_net_{name}"), getattr(a, f"critic_net_{name}"),
                              getattr(a, f"optimizer_actor_{name}"), getattr(a, f"optimizer_critic_{name}"),
                              b["obs"], b["act"], b["logp"], b["ret"], m, counts, per_row=kind == "d" and per_row))
    return heads


def _state(a):
    """Every net's flat weights and every optimiser's exp_avg, exp_avg_sq and step, on the host."""
    out = {}
    for n in NAMES:
        for k in ("actor", "critic"):
            net, opt = getattr(a, f"{k}_net_{n}"), getattr(a, f"optimizer_{k}_{n}")
            out[f"{k}_{n}.w"] = net.flat().detach().cpu().clone()
            for i, p in enumerate(net.parameters()):
                st = opt.state.get(p, {})
                for key in ("exp_avg", "exp_avg_sq", "step"):
                    if key in st:
                        out[f"{k}_{n}.{key}{i}"] = st[key].detach().cpu().clone()
    return out


def _assert_same(x, y):
    assert x.keys() == y.keys()
    bad = [k for k in x if not torch.equal(x[k], y[k])]
    assert not bad, bad


def _key_fn(e, i):
    return sr.shuffle_key(11, 5, e, i, 0)


@pytest.mark.parametrize("per_row,clip", [(False, None), (True, None), (False, 0.5)])
def test_minibatches_equal_train_epoch_on_permuted_slices(per_row, clip):
    from mhppo import ppo
    E, K = 2, 3
    a = _algo(0)
    buckets = _collect(a)
    assert all(buckets[n]["ret"].numel() > 4 * K for n in NAMES)
    res = ppo.train_minibatches(_heads(a, buckets, per_row), E, K, _key_fn, a.grad_bucket, clip)
    torch.cuda.synchronize()

    b = _algo(0)  # the same initial nets
    ref_norms = torch.full((E * K, 6), math.nan, dtype=torch.float64)
    last = None
    for e in range(E):
        perms = {n: torch.from_numpy(sr.perm(_key_fn(e, i), buckets[n]["ret"].numel())).to("cuda:0")
                 for i, n in enumerate(NAMES)}
        for j in range(K):
            rows = {}
            for n in NAMES:
                bd = sr.bounds(buckets[n]["ret"].numel(), K)
                rows[n] = perms[n][bd[j]:bd[j + 1]]
            heads = _heads(b, buckets, per_row, rows)
            assert all(h is not None for h in heads)
            nout = None if clip is None else torch.empty(6, dtype=torch.float64, device="cuda:0")
            last = ppo.train_epoch(heads, b.grad_bucket, clip, nout), [h.m for h in heads]
            if clip is not None:  # train_epoch: (actor, critic) per head; the driver: critics, then actors
                n6 = nout.cpu()
                ref_norms[e * K + j] = torch.cat([n6[1::2], n6[0::2]])
    torch.cuda.synchronize()
    _assert_same(_state(a), _state(b))
    losses = res[0] if clip is not None else res
    for (la, lc, m), (ra, rc), rm in zip(losses, last[0], last[1]):
        assert torch.equal(la, ra) and torch.equal(lc, rc) and m == rm
    if clip is not None:
        got = res[1].cpu()
        assert got.shape == (E * K, 6) and torch.equal(got, ref_norms) and bool(torch.isfinite(got).all())


def test_knob_off_never_reaches_the_shuffle(monkeypatch):
    from mhppo import _lib, ppo

    def boom(*a, **k):
        raise AssertionError("the minibatch path was reached with minibatches=None")

    monkeypatch.setattr(_lib, "batch_shuffle", boom)
    monkeypatch.setattr(ppo, "train_minibatches", boom)
    monkeypatch.setattr(_lib.lib(), "mhppo_batch_shuffle", boom)
    a = _algo(0)
    assert a.minibatches is None
    a.train(1)
    torch.cuda.synchronize()
    assert all(int(o.state_dict()["state"][0]["step"]) == 10 for o in a._optimizers().values())


def test_resume_is_bit_identical_and_steps_count(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    K = 4
    a = _algo(0, minibatches=K)
    a.train(2)
    b = _algo(0, minibatches=K)
    rows = _rows_seen(b)
    b.train(1)
    torch.cuda.synchronize()
    # every head has rows in each of its K slices here: 10 K steps per optimiser and iteration
    assert len(rows) == 1 and all(rows[0][n] >= 4 * K for n in NAMES)
    assert all(int(o.state_dict()["state"][0]["step"]) == 10 * K for o in b._optimizers().values())
    b.save_checkpoint("ck.pt")
    c = _algo(1234, minibatches=K)
    c.load_checkpoint("ck.pt")
    rows = _rows_seen(c)
    c.train(1)
    torch.cuda.synchronize()
    assert all(rows[0][n] >= 4 * K for n in NAMES)
    _assert_same(_state(a), _state(c))
    assert all(int(o.state_dict()["state"][0]["step"]) == 20 * K for o in c._optimizers().values())
    (ma, ia), (mc, ic) = a.venv.get_rng(), c.venv.get_rng()
    assert torch.equal(ma, mc) and torch.equal(ia, ic)
    assert a.curves() == c.curves()


def test_minibatches_change_the_update():
    a, b = _algo(0), _algo(0, minibatches=2)
    a.train(1)
    b.train(1)
    assert not torch.equal(a.actor_net_cross.flat(), b.actor_net_cross.flat())


def test_k_beyond_rows_over_4_skips_empty_slices():
    K = 40
    a = _algo(0, minibatches=K, max_grad_norm=math.inf)
    rows = _rows_seen(a)
    a.train(1)
    torch.cuda.synchronize()
    assert rows[0]["cross"] >= 4 * K and rows[0]["wait"] >= 4 * K
    bd = sr.bounds(rows[0]["choice"], K)
    on = [bd[j + 1] > bd[j] for j in range(K)]
    assert 0 < sum(on) < K  # the choice head has empty slices at this K
    for k in ("actor", "critic"):
        assert int(getattr(a, f"optimizer_{k}_choice").state_dict()["state"][0]["step"]) == 10 * sum(on)
        assert int(getattr(a, f"optimizer_{k}_cross").state_dict()["state"][0]["step"]) == 10 * K
    assert all(bool(torch.isfinite(n.flat()).all()) for n in a.nets())
    a.curves()
    entry = a.grad_norms[0]
    for k in ("actor", "critic"):
        got = entry[f"{k}_choice"]
        assert len(got) == 10 * K
        assert [not math.isnan(x) for x in got] == on * 10
        assert all(not math.isnan(x) for x in entry[f"{k}_cross"])


@pytest.mark.parametrize("bad", [0, -1, True, False, 2.0, "3"])
def test_constructor_refuses(bad):
    with pytest.raises(ValueError, match="minibatches"):
        _algo(0, minibatches=bad)
