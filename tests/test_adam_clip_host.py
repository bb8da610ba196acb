"""The clip-and-Adam contract on the host (no GPU needed): mhppo.ppo.adam_clip_torch, the executable
specification of mhppo_adam_clip (include/mhppo.h) and the CPU path of adam_steps(max_grad_norm=c),
against numpy restatements written here (fold order, per-element chain), against float64 torch
(accuracy, bounded by 4x the float32 torch path's own error: profiles/adam_clip/tolerance.txt),
Algo_PPO's validation of the knob, and the order all-reduce -> clip in train_epoch."""
import math

import numpy as np
import pytest
import torch

import adam_clip_common as C
import fold_ref as F

SIZES = sorted(set(F.EVS_N) | {sum(C.model_segs(*s)) for s in C.PRODUCT_NETS})


def _bits(a):
    return np.asarray(a, np.float64).reshape(-1).view(np.int64)


def _split(x, segs):
    out, off = [], 0
    for n in segs:
        out.append(x[off:off + n])
        off += n
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sum_of_squares_is_the_1024x4_fold(n):
    from mhppo import ppo
    g = F.heavy(np.random.default_rng(n), (33, n)).astype(np.float32)
    sq = g.astype(np.float64) ** 2
    ref = F.fold(sq, 1024, 4)
    for k in (0, 1, 32):  # as one tensor, and cut into ragged pieces (the flat index runs across them)
        cuts = [0, n // 3, n // 3, n - n // 5, n]
        parts = [torch.from_numpy(g[k, a:b]) for a, b in zip(cuts, cuts[1:])]
        assert _bits(ppo.adam_clip_sumsq([torch.from_numpy(g[k])]).item()) == _bits(ref[k])
        assert _bits(ppo.adam_clip_sumsq(parts).item()) == _bits(ref[k])
    if n >= 4095:  # the gradients tell the orders apart (below, a fourth chain of zeros hides the combine)
        for name, w in (("sequential", F.sequential(sq)), ("((a0+a1)+a2)+a3", F.fold(sq, 1024, 4, combine="left"))):
            d = int((_bits(ref) != _bits(w)).sum())
            print(f"n {n}: {name}: {d} of 33 sums differ")
            assert d >= 1, name


def _chain_numpy(p, g, m, v, s, a, q, c1, b2, c2, eps):
    """include/mhppo.h's per-element chain in numpy float32, one rounding per operation."""
    f = np.float32
    gs = g * f(s)
    m = m + (gs - m) * f(c1)
    v = v * f(b2) + (gs * gs) * f(c2)
    den = np.sqrt(v) / f(q) + f(eps)
    return p - f(a) * (m / den), m, v


@pytest.mark.parametrize("max_norm", [1.0, math.inf])
def test_per_element_chain_matches_numpy(max_norm):
    from mhppo import ppo
    rng = np.random.default_rng(7)
    segs = C.model_segs(13, 1)
    n = sum(segs)
    p0 = (0.1 * rng.standard_normal(n)).astype(np.float32)
    m0 = (0.01 * rng.standard_normal(n)).astype(np.float32)
    v0 = ((0.01 * rng.standard_normal(n)) ** 2).astype(np.float32)
    lr, b1, b2, eps = 3e-4, 0.9, 0.999, 1e-8
    p, m, v = (torch.from_numpy(x.copy()) for x in (p0, m0, v0))
    step = torch.tensor(4.0)
    pn, mn, vn = p0, m0, v0
    for t in (5, 6, 7):
        g = (F.heavy(rng, n) * 1e-3).astype(np.float32)
        views = [tuple(_split(x, segs)) for x in (p, torch.from_numpy(g), m, v)]
        norm = ppo.adam_clip_torch([(a, b, c, d, step) for a, b, c, d in zip(*views)], t, lr, b1, b2, eps, max_norm)
        want_norm = math.sqrt(float(F.fold(g.astype(np.float64) ** 2, 1024, 4)))
        assert norm == want_norm
        coef = max_norm / (want_norm + 1e-6)
        s = np.float32(coef) if coef < 1.0 else np.float32(1.0)
        assert (s < 1.0) == (max_norm == 1.0)  # heavy gradients: the finite bound clips, inf never does
        pn, mn, vn = _chain_numpy(pn, g, mn, vn, s, np.float32(lr / (1 - b1 ** t)), np.float32(math.sqrt(1 - b2 ** t)),
                                  np.float32(1 - b1), np.float32(b2), np.float32(1 - b2), np.float32(eps))
        for got, want in ((p, pn), (m, mn), (v, vn)):
            assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
        assert float(step) == t


def test_accuracy_against_float64():
    params, grads = C.accuracy_case()
    ref, ref_norms = C.torch_path(params, grads, torch.float64)
    for row in ref_norms:  # the bound straddles the nets' norms at every step
        assert any(x > C.ACC_MAX_NORM for x in row) and any(x < C.ACC_MAX_NORM for x in row), row
    f32, _ = C.torch_path(params, grads, torch.float32)
    spec, spec_norms = C.spec_path(params, grads)
    yard, got = C.worst_error(f32, ref), C.worst_error(spec, ref)
    print(f"float32 torch path {yard:.3e} (recorded {C.YARDSTICK_WORST:.3e}), contract {got:.3e}, "
          f"bound {4 * C.YARDSTICK_WORST:.3e}")
    assert got <= 4 * C.YARDSTICK_WORST
    for ra, rb in zip(spec_norms, ref_norms):  # float64 sums of ~5000 exact squares, in another order
        assert np.allclose(ra, rb, rtol=1e-13, atol=0)


def test_algo_validates_max_grad_norm():
    from mhppo.algo import Algo_PPO
    from mhppo.models import Model_PPO
    for bad in (0, 0.0, -1.0, float("nan"), -math.inf):
        with pytest.raises(ValueError, match="max_grad_norm"):
            Algo_PPO(Model_PPO, None, max_grad_norm=bad)  # raised before the env is touched
    algo = object.__new__(Algo_PPO)
    algo._init_hyperparameters({})
    assert algo.max_grad_norm is None
    for ok in (0.5, 1, 40.0, math.inf):
        algo._init_hyperparameters({"max_grad_norm": ok})
        assert algo.max_grad_norm == float(ok) and isinstance(algo.max_grad_norm, float)


def _cpu_nets(seed=3):
    from mhppo.models import Model_PPO
    torch.manual_seed(seed)
    nets = [Model_PPO(13, 1, 1, mean=-1.0, std=3.0), Model_PPO(13, 1, 0), Model_PPO(20, 2, 2)]
    opts = [torch.optim.Adam(n.parameters(), lr) for n, lr in zip(nets, (3e-4, 1e-3, 5e-4))]
    return nets, opts


def test_cpu_path_is_the_specification():
    from mhppo import ppo
    nets, opts = _cpu_nets()
    rng = np.random.default_rng(11)
    ref_p = [n.flat().clone() for n in nets]
    ref_m = [torch.zeros_like(x) for x in ref_p]
    ref_v = [torch.zeros_like(x) for x in ref_p]
    clipped = []
    for t in (1, 2, 3):
        grads = [torch.from_numpy((F.heavy(rng, n.flat().numel()) * sc).astype(np.float32))
                 for n, sc in zip(nets, (1e-7, 1e-2, 1e-3))]
        for n, g in zip(nets, grads):
            n.grad_flat().copy_(g)
        out = torch.full((3,), math.nan, dtype=torch.float64)
        assert ppo.adam_steps(opts, max_grad_norm=0.5, norms_out=out) is out
        for k, (n, o, lr) in enumerate(zip(nets, opts, (3e-4, 1e-3, 5e-4))):
            segs = C.model_segs(n.n_in, n.n_out)
            step = torch.zeros(())
            views = [_split(x, segs) for x in (ref_p[k], grads[k], ref_m[k], ref_v[k])]
            norm = ppo.adam_clip_torch([(a, b, c, d, step) for a, b, c, d in zip(*views)], t, lr, 0.9, 0.999, 1e-8, 0.5)
            clipped.append(norm > 0.5)
            assert float(out[k]) == norm
            assert torch.equal(n.flat().view(torch.int32), ref_p[k].view(torch.int32))
            st = [o.state[p] for p in n.parameters()]  # the torch optimiser's own state is what was stepped
            assert torch.equal(torch.cat([s["exp_avg"].reshape(-1) for s in st]), ref_m[k])
            assert torch.equal(torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]), ref_v[k])
            assert all(float(s["step"]) == t and s["step"].dtype == torch.float32 for s in st)
    assert any(clipped) and not all(clipped)
    # the state is torch's: a plain o.step() continues from it (step 4), and state_dict() carries it
    assert opts[0].state_dict()["state"][0]["step"] == 3
    ppo.clip_forget(opts)


def test_knob_off_takes_optimizer_step(monkeypatch):
    from mhppo import adam, ppo
    nets, opts = _cpu_nets()
    calls = []
    for o in opts:
        monkeypatch.setattr(o, "step", lambda o=o: calls.append(id(o)))
    reached = []  # replaced in mhppo.adam, where adam_steps looks the name up
    monkeypatch.setattr(adam, "adam_clip_steps", lambda *a, **k: reached.append(a))
    assert ppo.adam_steps is adam.adam_steps
    ppo.adam_steps(opts, max_grad_norm=0.5)  # the replacement is live: the knob reaches it
    assert len(reached) == 1 and calls == []
    assert ppo.adam_steps(opts) is None
    assert calls == [id(o) for o in opts]
    assert len(reached) == 1, "the clip path ran with the knob off"


def test_unsupported_optimizer_takes_the_torch_fallback():
    from mhppo import ppo
    nets, _ = _cpu_nets()
    opts = [torch.optim.Adam(nets[0].parameters(), 3e-4, weight_decay=0.01), torch.optim.SGD(nets[1].parameters(), 0.1)]
    ref = [n.flat().clone() for n in nets[:2]]
    for n in nets[:2]:
        n.grad_flat().copy_(torch.from_numpy(np.random.default_rng(2).standard_normal(n.flat().numel()).astype("f")))
    before = [float(n.grad_flat().double().norm()) for n in nets[:2]]
    norms = ppo.adam_steps(opts, max_grad_norm=0.5)
    for n, b, r in zip(nets[:2], before, norms.tolist()):
        assert b > 0.5 and abs(r - b) < 1e-5 * b  # the norm before clipping (float32, clip_grad_norm_'s)
        assert abs(float(n.grad_flat().double().norm()) - 0.5) < 1e-5  # clipped in place, as torch does
    want = ref[1] - 0.1 * nets[1].grad_flat()  # SGD on the clipped gradient
    assert torch.allclose(nets[1].flat(), want, rtol=0, atol=1e-6)
    assert not torch.equal(nets[0].flat(), ref[0])


def test_every_gradient_allreduce_precedes_the_clip(monkeypatch):
    """train_epoch / train_epochs under (forced) data parallelism with CPU doubles: within a step,
    the gradient all-reduce (float32 spans of the bucket) comes before the clip-and-Adam call."""
    from test_dp_gloo import _install_cpu_doubles
    from mhppo import ppo
    from mhppo.models import Model_PPO
    from mhppo import adam
    for name in ("k_adv_stats", "k_adv_normalize", "k_mse", "k_ppo_cont", "_critic_pass", "_actor_pass", "_pair_pass"):
        monkeypatch.setattr(ppo, name, getattr(ppo, name))  # restored after the test
    _install_cpu_doubles(ppo)
    events = []
    monkeypatch.setattr(ppo, "_dp", lambda: True)  # one rank: a SUM all-reduce is the identity
    monkeypatch.setattr(ppo.dist, "all_reduce",
                        lambda t, op=None: events.append("grad" if t.dtype == torch.float32 else "stats"))
    real = adam.adam_clip_steps  # replaced where adam_steps looks it up
    monkeypatch.setattr(adam, "adam_clip_steps", lambda *a, **k: (events.append("clip"), real(*a, **k))[1])
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    nets = [Model_PPO(13, 1, 1, mean=-1.0, std=3.0), Model_PPO(13, 1, 1, mean=-1.0, std=3.0), Model_PPO(13, 1, 0),
            Model_PPO(13, 1, 0)]
    bucket = ppo.GradBucket(nets, "cpu")
    opts = [torch.optim.Adam(n.parameters(), 3e-4) for n in nets]
    heads = []
    for h in range(2):
        M = 40 + h
        obs = torch.from_numpy(rng.normal(0, 3, (M, 13)).astype(np.float32))
        act, lp, ret = (torch.from_numpy(rng.normal(mu, 1, M).astype(np.float32)) for mu in (-1, -0.6, -20))
        heads.append(ppo.Head("c", nets[h], nets[2 + h], opts[h], opts[2 + h], obs, act, lp, ret, M))
    norms = torch.full((4,), math.nan, dtype=torch.float64)
    ppo.train_epoch(heads, bucket, max_grad_norm=0.5, norms_out=norms)
    assert events == ["stats", "grad", "clip"] and bool(torch.isfinite(norms).all())
    del events[:]
    losses, table = ppo.train_epochs(heads, 3, bucket, max_grad_norm=0.5)
    steps = "".join(e[0] for e in events).split("c")[:-1]  # one string of collectives per pipeline step
    assert len(steps) == 4 and all("g" in s for s in steps), events
    assert table.shape == (3, 4) and bool(torch.isfinite(table).all()) and len(losses) == 2
    ppo.clip_forget(opts)
