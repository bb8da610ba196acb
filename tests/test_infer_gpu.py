"""The batched head forward (mhppo_mlp_forward, Model_PPO.forward_rows) and the PPO diagnostics
(mhppo_ppo_diag, ppo.k_ppo_diag, Algo_PPO(diagnostics=True)) on the GPU, against the host harness
(tools/hostfwd.cpp: the same source compiled for the CPU) and against the rollout itself."""
import ctypes
import math

import numpy as np
import pytest
import torch

import infer_common as ic

pytestmark = pytest.mark.gpu
MS = (1, 31, 32, 33, 4099)  # one row, both sides of a tile edge, many blocks with a ragged tail


def gpu_net(kind, n_in, W):
    net = ic.make_net(kind, n_in, 0)
    net.load_packed(torch.from_numpy(np.asarray(W, np.float32)))
    return net.cuda()


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_head(c, Wa=None, Wc=None):
    from mhppo import ppo
    actor = gpu_net(c["akind"], c["n_in"], c["Wa"] if Wa is None else Wa)
    critic = gpu_net(0, c["n_in"], c["Wc"] if Wc is None else Wc)
    return ppo.Head("c" if c["akind"] == 1 else "d", actor, critic, None, None, t(c["X"]), t(c["act"]),
                    t(c["logp_old"]), t(c["ret"]), c["M"])


# ------------------------------------------------------------------ 1. forward vs the host harness
_FWD = {}


def _fwd_ref(kind, n_in):
    """Reference once per (kind, n_in) at the largest M; smaller M are its leading rows."""
    if (kind, n_in) not in _FWD:
        W = ic.packed_np(ic.make_net(kind, n_in, 40 + 7 * kind + n_in))
        X = ic.randn((max(MS), n_in), 90 + n_in)
        _FWD[(kind, n_in)] = (W, X, ic.hostfwd().forward(kind, W, X, ic.MEAN, ic.STD))
    return _FWD[(kind, n_in)]


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("n_in", ic.N_INS)
@pytest.mark.parametrize("kind", ic.KINDS)
def test_forward_bit_identical_to_host(kind, n_in, M):
    W, X, ref = _fwd_ref(kind, n_in)
    net = gpu_net(kind, n_in, W)
    out = net.forward_rows(t(X[:M]))
    assert out.shape == ((M, 2) if kind == 2 else (M,)) and out.dtype == torch.float32
    assert torch.equal(out.cpu(), torch.from_numpy(ref[:M]))


def test_forward_rows_rejects_what_it_cannot_run():
    net = gpu_net(1, 13, ic.packed_np(ic.make_net(1, 13, 1)))
    with pytest.raises(ValueError):
        net.forward_rows(torch.zeros(4, 12, device="cuda"))
    with pytest.raises(ValueError):
        net.forward_rows(torch.zeros(4, 13, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        net.forward_rows(torch.zeros(4, 13))
    assert net.forward_rows(torch.zeros(0, 13, device="cuda")).shape == (0,)
    # a non-contiguous / unaligned view is taken as it is
    X = t(ic.randn((40, 14), 3))
    assert torch.equal(net.forward_rows(X[:, 1:]), net.forward_rows(X[:, 1:].contiguous()))


# ------------------------------------------------------------------ 2. forward vs the rollout
def _collect(variant, nc, npd, nl, N=64):
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    from mhppo.rollout import RolloutGPU
    venv = VecCrosswalk(variant, N, nc, npd, nl, seed_base=4100)
    ro = RolloutGPU(venv)
    torch.manual_seed(21)
    ac = Model_PPO(13, 1, 1, mean=ic.MEAN, std=ic.STD).cuda()
    aw = Model_PPO(13, 1, 1, mean=ic.MEAN, std=ic.STD).cuda()
    ad = Model_PPO(ro.dc, 2, 2).cuda()
    cc, cw, cd = (Model_PPO(13, 1, 0).cuda(), Model_PPO(13, 1, 0).cuda(), Model_PPO(ro.dc, 1, 0).cuda())
    batch = ro.collect(ac, aw, ad, seed=9, iteration=0)
    torch.cuda.synchronize()
    return ro, batch, (ac, aw, ad), (cc, cw, cd)


def _assert_zero_diag(head, what):
    from mhppo import ppo
    M = head.obs.shape[0]
    assert M > 0, what
    s = ppo.k_ppo_diag(head).tolist()
    print(f"{what}: M {M} sums {s}")
    assert s[ppo.DIAG_DSUM] == 0.0 and s[ppo.DIAG_K3] == 0.0 and s[ppo.DIAG_CLIP] == 0.0, what
    assert s[ppo.DIAG_RATIO] == float(M), what


@pytest.mark.parametrize("case", [("coop", 4, 3, 2), ("4cars", 4, 1, 2)], ids=["coop_4_3_2", "4cars_4_1_2"])
def test_forward_reproduces_rollout(case):
    """Every recorded log-probability is mvn_logp(act, forward_rows(obs_c row)) of the head that
    acted, bit for bit, and forward_rows(feat_d) the recorded choice probabilities; the diagnostics
    with the collecting weights then see d == 0 in every row.

    The head that acted on a record is the one chosen by a_d of the (slot, SELECTED pedestrian)
    row (k_policy_mfma heads by (env, slot, ped) row; k_sample_env records the pedestrian with the
    smallest output).  With one pedestrian (4cars 4/1/2) that is the bucket rule's head
    (a_d[env].flat[slot], tests/test_policy_torch_gpu.py), asserted for every record and through
    the bucketed heads.  With three (coop 4/3/2) the bucket rule indexes the per-(car, ped) array
    by the car index (the reference's own behaviour), which can name another head than
    the one that acted (measured here: on 5 324 of the 20 480 records): there the acting head is
    known where a slot's three choices agree (13 600 records) — those
    records are asserted against that head alone and make up the diagnostics' heads — and every
    other record must match one of the two heads."""
    from mhppo import ppo
    from mhppo.rollout import bucket_segments
    hf = ic.hostfwd()
    ro, batch, (ac, aw, ad), (cc, cw, cd) = _collect(*case)
    N, S, P, T = batch.N, batch.S, batch.P, batch.T
    # choice head
    feat_d = batch.feat_d.reshape(N * S * P, -1)
    assert torch.equal(ad.forward_rows(feat_d), batch.probs_d.reshape(N * S * P, 2))
    # continuous heads: records [N, S, T]
    obs = batch.obs_c.reshape(N * S * T, 13).contiguous()
    act = batch.act.reshape(-1).contiguous()
    logp = batch.logp.reshape(-1).contiguous()
    two = torch.tensor(2.0, device="cuda")
    lp = [torch.from_numpy(hf.mvn_logp(act.cpu().numpy(), torch.minimum(net.forward_rows(obs), two).cpu().numpy()))
          for net in (ac, aw)]
    rec = logp.cpu()
    a = batch.a_d.reshape(N, S, P).cpu()
    agree = (a == a[:, :, :1]).all(-1)                      # [N, S]: the slot's pedestrians chose alike
    strict = agree.reshape(N * S, 1).expand(N * S, T).reshape(-1)
    wait = (a[:, :, 0] == 1).reshape(N * S, 1).expand(N * S, T).reshape(-1)   # action_d = 2a - 1 > 0
    acting = torch.where(wait, lp[1], lp[0])
    assert strict.sum() > 0
    assert torch.equal(acting[strict], rec[strict])
    either = (lp[0] == rec) | (lp[1] == rec)
    rule_wait = (a.reshape(N, S * P)[:, :S] == 1).reshape(N * S, 1).expand(N * S, T).reshape(-1)
    off_rule = int((torch.where(rule_wait, lp[1], lp[0]) != rec).sum())
    print(f"{case}: {int(strict.sum())} of {strict.numel()} records with a known acting head; "
          f"{off_rule} records whose bucket-rule head did not act")
    assert bool(either.all())
    cross, wait_b, choice = bucket_segments(batch)
    if P == 1:
        assert bool(strict.all())
        # the bucket rule's head is the acting head: the bucketed heads as update() builds them
        _assert_zero_diag(ppo.Head("c", ac, cc, None, None, cross["obs"], cross["act"], cross["logp"], cross["ret"],
                                   cross["ret"].numel()), "cross bucket")
        _assert_zero_diag(ppo.Head("c", aw, cw, None, None, wait_b["obs"], wait_b["act"], wait_b["logp"],
                                   wait_b["ret"], wait_b["ret"].numel()), "wait bucket")
    else:
        ret = torch.zeros_like(act)
        for net, crit, sel, what in ((ac, cc, strict & ~wait, "cross records"), (aw, cw, strict & wait, "wait records")):
            idx = torch.nonzero(sel).flatten().cuda()
            _assert_zero_diag(ppo.Head("c", net, crit, None, None, obs[idx], act[idx], logp[idx], ret[idx], idx.numel()),
                              what)
    _assert_zero_diag(ppo.Head("d", ad, cd, None, None, choice["obs"], choice["act"], choice["logp"], choice["ret"],
                               choice["ret"].numel()), "choice bucket")


def test_forward_reproduces_rollout_choice_scalable():
    """Scalable 8/1/4 (dc = 54): the choice probabilities only (an absent pedestrian leaves
    loc = 2.0, which is no head output)."""
    ro, batch, (ac, aw, ad), _ = _collect("scalable", 8, 1, 4)
    R = batch.N * batch.S * batch.P
    assert ro.dc == 54
    assert torch.equal(ad.forward_rows(batch.feat_d.reshape(R, -1)), batch.probs_d.reshape(R, 2))


# ------------------------------------------------------------------ 3. sums vs the host harness
# seeds for which the reference's rows keep clear of the clip boundaries (asserted below)
DIAG_CASES = [(1, 13, 0.05, 1, 5014), (1, 13, 0.05, 33, 5046), (1, 13, 0.05, 4099, 9112),
              (2, 27, 0.1, 1, 5028), (2, 27, 0.1, 33, 5060), (2, 27, 0.1, 4099, 6200),
              (2, 54, 0.1, 33, 5087), (2, 64, 0.1, 4099, 6000)]  # the wide heads: LDS above 64 KB


@pytest.mark.parametrize("akind,n_in,sigma,M,seed", DIAG_CASES)
def test_diag_sums_vs_host(akind, n_in, sigma, M, seed):
    from mhppo import ppo
    c = ic.diag_case(akind, n_in, M, sigma, seed)
    d, terms, lp = ic.host_terms(c)
    if M >= 33:  # the reference alone: a real mix of clipped rows, none at a boundary
        frac = terms[:, 2].mean()
        near = min(np.abs(d - ic.LN_0_8).min(), np.abs(d - ic.LN_1_2).min())
        print(f"reference clip fraction {frac:.3f}, nearest row to a boundary {near:.3g}")
        assert 0.05 <= frac <= 0.95
        assert near > 1e-6
    got = ppo.k_ppo_diag(make_head(c)).cpu().numpy()
    want, scale = terms.sum(0), np.abs(terms).sum(0)
    slack = 2.0 ** -22 * np.abs(lp.astype(np.float64)).sum() if akind == 2 else 0.0  # logf: <= 1 ulp each side
    for k in range(10):
        print(f"term {k}: gpu {got[k]!r} host {want[k]!r} sum |term| {scale[k]:.3g}")
    assert got[ppo.DIAG_CLIP] == want[ppo.DIAG_CLIP]
    for k in (ppo.DIAG_DSUM, ppo.DIAG_K3, ppo.DIAG_RATIO):
        assert abs(got[k] - want[k]) <= slack + 1e-10 * scale[k], k
    for k in (ppo.DIAG_ENT, ppo.DIAG_E, ppo.DIAG_E2, ppo.DIAG_G, ppo.DIAG_G2, ppo.DIAG_V):
        assert abs(got[k] - want[k]) <= 1e-10 * scale[k], k
    if akind == 1:
        assert got[ppo.DIAG_ENT] == 0.0


# ------------------------------------------------------------------ 4. determinism, streams, shards
@pytest.mark.parametrize("akind,n_in,sigma,seed", [(1, 13, 0.05, 9112), (2, 27, 0.1, 6200)])
def test_diag_deterministic_streams_and_shards(akind, n_in, sigma, seed):
    from mhppo import ppo
    M, a = 4099, 1000
    c = ic.diag_case(akind, n_in, M, sigma, seed)
    h = make_head(c)
    s1 = ppo.k_ppo_diag(h)
    s2 = ppo.k_ppo_diag(h)
    assert torch.equal(s1, s2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s3 = ppo.k_ppo_diag(h)
    side.synchronize()
    assert torch.equal(s1, s3)
    # two shards add up to the whole (the data-parallel contract)
    parts = []
    for lo, hi in ((0, a), (a, M)):
        hp = ppo.Head(h.kind, h.actor, h.critic, None, None, h.obs[lo:hi], h.act[lo:hi], h.logp[lo:hi], h.ret[lo:hi],
                      M)
        parts.append(ppo.k_ppo_diag(hp).cpu().numpy())
    _, terms, _ = ic.host_terms(c)
    scale = np.abs(terms).sum(0)
    whole = s1.cpu().numpy()
    assert np.all(np.abs(parts[0] + parts[1] - whole) <= 1e-12 * scale)


# ------------------------------------------------------------------ 5. errors
def test_einval_and_empty():
    from mhppo import _lib, ppo
    L = _lib.lib()
    c = ic.diag_case(1, 13, 8, 0.0, 77)
    h = make_head(c)
    sums = torch.full((ppo.DIAG_N,), 7.0, dtype=torch.float64, device="cuda")
    work = torch.empty(64, dtype=torch.float64, device="cuda")
    out = torch.empty(8, device="cuda")
    p, st = _lib.ptr, _lib.stream_ptr()

    def fwd(d, X=h.obs, o=out, M=8):
        return L.mhppo_mlp_forward(ctypes.byref(d), p(X), M, p(o), st)

    def diag(da, dc, X=h.obs, act=h.act, lp=h.logp, ret=h.ret, s=sums, w=work, M=8):
        return L.mhppo_ppo_diag(ctypes.byref(da), ctypes.byref(dc), p(X), M, p(act), p(lp), p(ret), p(s), p(w), st)

    def desc(net, **kw):
        d, keep = net.mlp_desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    da, dc = desc(h.actor), desc(h.critic)
    assert fwd(da) == 0 and diag(da, dc) == 0
    cases = [
        (lambda: fwd(desc(h.actor, n_in=65)), "n_in 65"),
        (lambda: fwd(desc(h.actor, n_in=0)), "n_in 0"),
        (lambda: fwd(desc(h.actor, n_out=2)), "needs n_out 1"),
        (lambda: fwd(desc(h.actor, kind=2)), "needs n_out 2"),
        (lambda: fwd(desc(h.actor, kind=3)), "kind 3"),
        (lambda: fwd(da, X=None), "null pointer"),
        (lambda: fwd(da, o=None), "null pointer"),
        (lambda: fwd(desc(h.actor, packed=None)), "null pointer"),
        (lambda: diag(desc(h.actor, n_in=65), desc(h.critic, n_in=65)), "n_in 65"),
        (lambda: diag(da, desc(h.critic, n_in=12)), "actor n_in 13 != critic n_in 12"),
        (lambda: diag(dc, dc), "the actor is kind 0"),
        (lambda: diag(da, da), "the critic is kind 1"),
        (lambda: diag(desc(h.actor, n_out=2), dc), "needs n_out 1"),
        (lambda: diag(da, dc, act=None), "null pointer"),
        (lambda: diag(da, dc, lp=None), "null pointer"),
        (lambda: diag(da, dc, ret=None), "null pointer"),
        (lambda: diag(da, dc, X=None), "null pointer"),
        (lambda: diag(da, dc, w=None), "null pointer"),
        (lambda: diag(da, dc, s=None), "null pointer"),
        (lambda: diag(da, dc, M=-1), "M < 0"),
    ]
    for call, msg in cases:
        with pytest.raises(_lib.MhppoError) as e:
            _lib.check(call())
        assert "error -1" in str(e.value) and msg in str(e.value), (msg, str(e.value))
    # M == 0: zeros, nothing else (the data pointers may be NULL)
    assert diag(da, dc, X=None, act=None, lp=None, ret=None, w=None, M=0) == 0
    torch.cuda.synchronize()
    assert torch.equal(sums.cpu(), torch.zeros(ppo.DIAG_N, dtype=torch.float64))
    assert fwd(da, X=None, o=None, M=0) == 0
    empty = ppo.Head("c", h.actor, h.critic, None, None, h.obs[:0], h.act[:0], h.logp[:0], h.ret[:0], 8)
    assert torch.equal(ppo.k_ppo_diag(empty).cpu(), torch.zeros(ppo.DIAG_N, dtype=torch.float64))
    with pytest.raises(ValueError):
        ppo.k_ppo_diag(ppo.Head("d", h.actor, h.critic, None, None, h.obs, h.act, h.logp, h.ret, 8))


# ------------------------------------------------------------------ 6. Algo_PPO
def _train(n, **kw):
    from mhppo import ppo
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    venv = VecCrosswalk("4cars", 256, 4, 1, 2, seed_base=0)
    torch.manual_seed(0)
    algo = Algo_PPO(Model_PPO, venv, verbose=False, save_curves=False, **kw)
    direct = []
    reset = algo.rollout.reset

    def spy():  # the trailing reset of an iteration: the buckets are still there
        r = algo.rollout
        if kw.get("diagnostics") and r.cross is not None:
            entry = {}
            for name, kind, b in (("cross", "c", r.cross), ("wait", "c", r.wait), ("choice", "d", r.choice)):
                m = b["ret"].numel()
                if m > 0:
                    h = ppo.Head(kind, getattr(algo, f"actor_net_{name}"), getattr(algo, f"critic_net_{name}"), None, None,
                                 b["obs"], b["act"], b["logp"], b["ret"], m)
                    entry[name] = ppo.diag_stats(ppo.k_ppo_diag(h).tolist(), m, entropy=(kind == "d"))
            direct.append(entry)
        reset()

    algo.rollout.reset = spy
    algo.train(n)
    torch.cuda.synchronize()
    return algo, direct


def test_algo_diagnostics():
    off, _ = _train(2)
    on, direct = _train(2, diagnostics=True)
    assert off.diagnostics == [] and not off._pending_diag
    for a, b in zip(off.nets(), on.nets()):  # no behaviour change
        assert torch.equal(a.flat(), b.flat())
    assert off.curves() == on.curves()
    D = on.diagnostics
    assert [e["iteration"] for e in D] == [0, 1] and len(direct) == 2
    for e, balance in zip(D, on.ep_scenario_balance):
        want = {"iteration", "choice"} | ({"cross"} if balance[0] else set()) | ({"wait"} if balance[1] else set())
        assert set(e) == want
        for name in want - {"iteration"}:
            st = e[name]
            assert all(math.isfinite(v) for v in st.values()), (name, st)
            assert st["approx_kl"] >= 0.0 and 0.0 <= st["clip_frac"] <= 1.0 and st["value_mse"] >= 0.0
            assert ("entropy" in st) == (name == "choice")
        assert 0.0 < e["choice"]["entropy"] <= math.log(2.0)
    last = dict(D[-1])
    assert last.pop("iteration") == 1
    assert last == direct[-1]
    # the update moved the policy: after ten epochs the batch no longer has ratio 1 everywhere
    assert any(e[k]["approx_kl"] > 0.0 for e in D for k in e if k != "iteration")


def test_algo_diagnostics_every():
    on, _ = _train(2, diagnostics=True, diagnostics_every=2)
    assert [e["iteration"] for e in on.diagnostics] == [0]
