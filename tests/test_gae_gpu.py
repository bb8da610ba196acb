"""GAE(lambda) targets on the GPU: mhppo_gae_tm (csrc/mlp_gae.hip) through mhppo.rollout
.gae_targets_tm, bucket_segments(gae=...) and Algo_PPO(gae_lambda=...).

The values the scan uses are checked bit for bit against Model_PPO.forward_rows and the host
harness (tools/hostfwd: the device source compiled for the CPU); the targets bit for bit against
include/mhppo.h's recurrence in numpy float64 from those values."""
import ctypes
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import infer_common as ic

pytestmark = pytest.mark.gpu

T_MAX, B_MAX = 80, 4133
GL = ((0.99, 0.95), (0.99, 1.0), (0.99, 0.0), (1.0, 1.0))
PATTERNS = ("none", "all0", "all1", "alt", "runs32", "rand30", "tile_off")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_critic(n_in, W):
    net = ic.make_net(0, n_in, 0)
    net.load_packed(torch.from_numpy(np.asarray(W, np.float32)))
    return net.cuda()


def critic_weights(n_in, seed):
    """A critic's packed weights, perturbed so that |V| is of the order of 1 on N(0, 1) rows (the
    fresh initialisation gives |V| ~ 0.1: the scan's V terms would hide behind the rewards)."""
    return ic.perturbed(ic.packed_np(ic.make_net(0, n_in, seed)), 0.2, seed + 1)


def ref_ret(rew, val, used, gamma, lam):
    """include/mhppo.h's recurrence, op for op, in numpy float64: rew [T, B] float64, val [T, B]
    float32 (the record's critic's output) -> float32 [T, B], 0 for unused records."""
    T, B = rew.shape
    out = np.zeros((T, B), np.float32)
    nv, A, c = np.zeros(B), np.zeros(B), gamma * lam
    for s in range(T - 1, -1, -1):
        v = val[s].astype(np.float64)
        d = (rew[s] + gamma * nv) - v
        A = d + c * A
        out[s] = (A + v).astype(np.float32)
        nv = v
    out[:, ~used] = 0.0
    return out


def pattern(name, B, seed=0):
    """(pos int64 [B] or None, bucket int8 [B] or None, used bool [B], b1 bool [B])."""
    rng = np.random.default_rng(1000 + seed)
    idx = np.arange(B)
    used = np.ones(B, bool)
    if name == "none":
        return None, None, used, np.zeros(B, bool)
    if name == "all0":
        b1 = np.zeros(B, bool)
    elif name == "all1":
        b1 = np.ones(B, bool)
    elif name == "alt":
        b1 = (idx & 1) == 1
    elif name == "runs32":  # whole tiles of one bucket: the other critic's forward is skipped
        b1 = ((idx >> 5) & 1) == 1
    elif name == "rand30":
        b1 = rng.random(B) < 0.5
        used = rng.random(B) >= 0.3
    elif name == "tile_off":  # one whole tile without a used record (the second; the only one if B <= 32)
        b1 = rng.random(B) < 0.5
        if B > 32:
            used[32:64] = False
        else:
            used[:] = False
    else:
        raise ValueError(name)
    pos = np.where(used, np.cumsum(used) - 1, -1).astype(np.int64)
    # an unused record's bucket entry is whatever the plan left there: it must not matter
    bucket = np.where(used, b1, rng.random(B) < 0.5).astype(np.int8)
    return pos, bucket, used, b1 & used


_DATA = {}


def dataset(n_in):
    """Once per n_in at the largest (T, B): observations, rewards, two critics, and the host
    harness's values of both over every one of the 330 640 rows (the scalar CPU forward takes 13 us
    a row: the steps are forwarded by a few threads, the harness is a pure function and ctypes
    releases the interpreter lock).  Smaller cases are leading slices."""
    if n_in not in _DATA:
        rng = np.random.default_rng(70 + n_in)
        X = rng.standard_normal((T_MAX, B_MAX, n_in)).astype(np.float32)
        rew = rng.standard_normal((T_MAX, B_MAX))
        W = [critic_weights(n_in, 500 + n_in), critic_weights(n_in, 600 + n_in)]
        hf = ic.hostfwd()
        with ThreadPoolExecutor(8) as pool:
            V = [np.stack(list(pool.map(lambda x, w=w: hf.forward(0, w, x), X))) for w in W]
        print(f"n_in {n_in}: mean |V| {np.abs(V[0]).mean():.3f} / {np.abs(V[1]).mean():.3f}")
        _DATA[n_in] = dict(X=X, rew=rew, W=W, V=V, nets=[gpu_critic(n_in, w) for w in W])
    return _DATA[n_in]


def run(nets, X, rew, pos, bucket, gamma, lam):
    from mhppo.rollout import gae_targets_tm
    ret, val = gae_targets_tm(X, rew, nets[0], nets[1], None if pos is None else t(pos),
                              None if bucket is None else t(bucket), gamma, lam, want_value=True)
    return ret.cpu().numpy(), val.cpu().numpy()


# ------------------------------------------------------------------ 1. values and targets
@pytest.mark.parametrize("B", (1, 33, 200, 4133))
@pytest.mark.parametrize("T", (1, 2, 80))
@pytest.mark.parametrize("n_in", (13, 27))
def test_values_and_targets_bit_identical(n_in, T, B):
    D = dataset(n_in)
    Xn, rn = np.ascontiguousarray(D["X"][:T, :B]), np.ascontiguousarray(D["rew"][:T, :B])
    X, rew = t(Xn), t(rn)
    # the host harness's values of the same rows, and forward_rows of them, agree
    Vh = [v[:T, :B] for v in D["V"]]
    for net, v in zip(D["nets"], Vh):
        assert np.array_equal(net.forward_rows(X.reshape(T * B, n_in)).reshape(T, B).cpu().numpy(), v)
    for name in PATTERNS:
        pos, bucket, used, b1 = pattern(name, B, seed=B + T)
        want_val = np.where(used[None, :], np.where(b1[None, :], Vh[1], Vh[0]), np.float32(0.0))
        for k, (gamma, lam) in enumerate(GL):
            ret, val = run(D["nets"], X, rew, pos, bucket, gamma, lam)
            what = (name, gamma, lam)
            assert np.array_equal(val, want_val), what
            assert np.array_equal(ret, ref_ret(rn, want_val, used, gamma, lam)), what
            assert not ret[:, ~used].any() and not val[:, ~used].any(), what
            if k == 0 and not used.all():
                # anything in an unused record's observation rows, NaN included, changes no bit
                Xp = X.clone()
                Xp[:, t(~used)] = float("nan")
                ret2, val2 = run(D["nets"], Xp, rew, pos, bucket, gamma, lam)
                assert np.array_equal(ret2, ret) and np.array_equal(val2, val), what


def test_without_value_output_and_one_critic():
    from mhppo.rollout import gae_targets_tm
    D = dataset(13)
    X, rew = t(D["X"][:7, :200]), t(D["rew"][:7, :200])
    ret, val = gae_targets_tm(X, rew, D["nets"][0], gamma=0.99, lam=0.95, want_value=True)
    only = gae_targets_tm(X, rew, D["nets"][0], gamma=0.99, lam=0.95)
    assert only.shape == rew.shape and only.dtype == torch.float32
    assert torch.equal(only, ret)
    assert np.array_equal(val.cpu().numpy(), D["V"][0][:7, :200])
    # records in any leading shape: [T, N, S]
    r3 = gae_targets_tm(X.reshape(7, 50, 4, 13), rew.reshape(7, 50, 4), D["nets"][0], gamma=0.99, lam=0.95)
    assert r3.shape == (7, 50, 4) and torch.equal(r3.reshape(7, 200), ret)


# the launch shapes (csrc/mlp_gae.hip launch): up to 1024 tiles a tile is served by two waves, one
# per critic (all of the cases above; with pos = None never), beyond by one wave, which walks the
# tiles grid-stride past 2048; n_in 64: dynamic LDS above 64 KB.  The values here are forward_rows'
# (checked against the host harness above and in test_infer_gpu.py).
@pytest.mark.parametrize("n_in,B", [(13, 1024 * 32), (13, 1024 * 32 + 1), (13, 2048 * 32 + 33), (64, 200),
                                    (64, 2048 * 32 + 33)])
def test_launch_shapes(n_in, B):
    T = 3
    rng = np.random.default_rng(n_in + B)
    Xn = rng.standard_normal((T, B, n_in)).astype(np.float32)
    rn = rng.standard_normal((T, B))
    nets = [gpu_critic(n_in, critic_weights(n_in, 700 + n_in)), gpu_critic(n_in, critic_weights(n_in, 800 + n_in))]
    X, rew = t(Xn), t(rn)
    Vg = [net.forward_rows(X.reshape(T * B, n_in)).reshape(T, B).cpu().numpy() for net in nets]
    for name in ("none", "rand30", "runs32"):
        pos, bucket, used, b1 = pattern(name, B)
        want_val = np.where(used[None, :], np.where(b1[None, :], Vg[1], Vg[0]), np.float32(0.0))
        ret, val = run(nets, X, rew, pos, bucket, 0.99, 0.95)
        assert np.array_equal(val, want_val), name
        assert np.array_equal(ret, ref_ret(rn, want_val, used, 0.99, 0.95)), name


# ------------------------------------------------------------------ 2. determinism
def test_streams_and_split_batches():
    D = dataset(13)
    B, T, cut = B_MAX, T_MAX, 2048
    X, rew = t(D["X"]), t(D["rew"])
    pos, bucket, used, b1 = pattern("rand30", B)
    a = run(D["nets"], X, rew, pos, bucket, 0.99, 0.95)
    b = run(D["nets"], X, rew, pos, bucket, 0.99, 0.95)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run(D["nets"], X, rew, pos, bucket, 0.99, 0.95)
    side.synchronize()
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    # the batch split at a multiple of 32 records
    parts = [run(D["nets"], X[:, lo:hi].contiguous(), rew[:, lo:hi].contiguous(), pos[lo:hi], bucket[lo:hi], 0.99, 0.95)
             for lo, hi in ((0, cut), (cut, B))]
    for k in range(2):
        assert np.array_equal(np.concatenate([parts[0][k], parts[1][k]], 1), a[k])


# ------------------------------------------------------------------ 3. errors
def test_einval_and_empty():
    from mhppo import _lib
    from mhppo.rollout import gae_targets_tm
    L = _lib.lib()
    D = dataset(13)
    T, B = 4, 40
    X, rew = t(D["X"][:T, :B]), t(D["rew"][:T, :B])
    pos_n, bucket_n, _, _ = pattern("alt", B)
    pos, bucket = t(pos_n), t(bucket_n)
    ret = torch.full((T, B), 7.0, device="cuda")
    val = torch.full((T, B), 7.0, device="cuda")
    p, st = _lib.ptr, _lib.stream_ptr()
    actor = ic.make_net(1, 13, 3).cuda()
    wide = gpu_critic(27, critic_weights(27, 9))

    def desc(net, **kw):
        d, keep = net.mlp_desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    c0, c1 = desc(D["nets"][0]), desc(D["nets"][1])

    def call(d0=c0, d1=c1, X=X, rew=rew, pos=pos, bucket=bucket, B=B, T=T, gamma=0.99, lam=0.95, ret=ret, val=val):
        ref = lambda d: ctypes.byref(d) if d is not None else None
        return L.mhppo_gae_tm(ref(d0), ref(d1), p(X), p(rew), p(pos), p(bucket), B, T, gamma, lam, p(ret), p(val), st)

    nan = float("nan")
    cases = [
        (lambda: call(d0=None), "null pointer (critic0)"),
        (lambda: call(d0=desc(D["nets"][0], packed=None)), "null pointer (critic0)"),
        (lambda: call(d1=None), "null pointer (critic1)"),
        (lambda: call(X=None), "null pointer"),
        (lambda: call(rew=None), "null pointer"),
        (lambda: call(ret=None), "null pointer"),
        (lambda: call(T=0), "T < 1"),
        (lambda: call(B=-1), "B < 0"),
        (lambda: call(d0=desc(actor)), "critic0 is kind 1"),
        (lambda: call(d1=desc(actor)), "critic1 is kind 1"),
        (lambda: call(d0=desc(D["nets"][0], n_in=0), d1=desc(D["nets"][1], n_in=0)), "n_in 0 outside"),
        (lambda: call(d0=desc(D["nets"][0], n_in=65), d1=desc(D["nets"][1], n_in=65)), "n_in 65 outside"),
        (lambda: call(d1=desc(wide)), "critic0 n_in 13 != critic1 n_in 27"),
        (lambda: call(d1=desc(wide), pos=None, bucket=None), "critic0 n_in 13 != critic1 n_in 27"),
        (lambda: call(bucket=None), "pos without bucket"),
        (lambda: call(gamma=-0.01), "gamma outside"),
        (lambda: call(gamma=1.01), "gamma outside"),
        (lambda: call(gamma=nan), "gamma outside"),
        (lambda: call(lam=-0.01), "lambda outside"),
        (lambda: call(lam=1.01), "lambda outside"),
        (lambda: call(lam=nan), "lambda outside"),
    ]
    for fn, msg in cases:
        with pytest.raises(_lib.MhppoError) as e:
            _lib.check(fn())
        assert "error -1" in str(e.value) and msg in str(e.value), (msg, str(e.value))
    torch.cuda.synchronize()
    assert bool((ret == 7.0).all()) and bool((val == 7.0).all())  # nothing was launched
    # B == 0: OK, nothing launched (the data pointers may be NULL)
    assert call(B=0) == 0 and call(B=0, X=None, rew=None, pos=None, bucket=None, ret=None, val=None) == 0
    torch.cuda.synchronize()
    assert bool((ret == 7.0).all())
    e = gae_targets_tm(X[:, :0], rew[:, :0], D["nets"][0])
    assert e.shape == (T, 0)
    # pos == NULL: critic1 and bucket may be NULL; value_tm may be NULL
    assert call(d1=None, pos=None, bucket=None, val=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ret.cpu().numpy(),
                          ref_ret(D["rew"][:T, :B], D["V"][0][:T, :B], np.ones(B, bool), 0.99, 0.95))
    assert bool((val == 7.0).all())
    # the wrapper refuses what the kernel could not index
    with pytest.raises(ValueError):
        gae_targets_tm(X[..., :12], rew, D["nets"][0])
    with pytest.raises(ValueError):
        gae_targets_tm(X, rew, D["nets"][0], D["nets"][1], pos[:-1], bucket[:-1])
    with pytest.raises(ValueError):
        gae_targets_tm(X, rew, D["nets"][0], None, pos, bucket)
    with pytest.raises(ValueError):
        gae_targets_tm(X, rew.float(), D["nets"][0])


# ------------------------------------------------------------------ 4. through the stack
STACK = {"coop_2_1_2": ("coop", 2, 1, 2), "scalable_8_1_4": ("scalable", 8, 1, 4)}
REC = ("obs", "act", "logp", "rew")


def _algo(case, N=64, **kw):
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    variant, nc, npd, nl = STACK[case]
    venv = VecCrosswalk(variant, N, nc, npd, nl, seed_base=77)
    torch.manual_seed(5)
    return Algo_PPO(Model_PPO, venv, verbose=False, save_curves=False, **kw)


_ROLL = {}


def _rollout(case, lam):
    """One rollout.reset() + iterations_rand from a fixed seed with rollout.gae set for `lam` (None:
    off); the same seed gives the same episode, so the runs differ in the targets alone."""
    if (case, lam) not in _ROLL:
        algo = _algo(case)
        r = algo.rollout
        r.gae = None if lam is None else (algo.critic_net_cross, algo.critic_net_wait, 0.99, lam)
        r.reset()
        r.iterations_rand(algo.actor_net_cross, algo.actor_net_wait, algo.actor_net_choice)
        torch.cuda.synchronize()
        _ROLL[(case, lam)] = algo
    return _ROLL[(case, lam)]


def _same(a, b, keys):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


def _ulp_apart(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("case", list(STACK))
def test_buckets_hold_the_lambda_returns(case):
    off, on = _rollout(case, None), _rollout(case, 0.95)
    ro, rn = off.rollout, on.rollout
    T = rn.batch.T
    if case.startswith("scalable"):  # the compact record layout with absent slots
        assert rn.batch.rec_of is not None and int((rn.batch.rec_of < 0).sum()) > 0
    total = 0
    for name, critic in (("cross", on.critic_net_cross), ("wait", on.critic_net_wait)):
        b0, b1 = getattr(ro, name), getattr(rn, name)
        assert b0["n_seg"] == b1["n_seg"]
        _same(b0, b1, REC)
        n = b1["n_seg"]
        total += n
        if n == 0:
            assert b1["ret"].numel() == 0
            continue
        v = critic.forward_rows(b1["obs"]).reshape(n, T).cpu().numpy()
        rew = b1["rew"].reshape(n, T).cpu().numpy()
        want = ref_ret(np.ascontiguousarray(rew.T), np.ascontiguousarray(v.T), np.ones(n, bool), 0.99, 0.95).T
        assert np.array_equal(b1["ret"].reshape(n, T).cpu().numpy(), want), name
        assert not torch.equal(b0["ret"], b1["ret"]), name
    assert total > 0
    _same(ro.choice, rn.choice, ("obs", "act", "logp", "ret", "counts", "rew_sums"))
    assert ro.choice["n_seg"] == rn.choice["n_seg"]


@pytest.mark.parametrize("case", list(STACK))
def test_lambda_one_is_the_default_target(case):
    """lam = 1 against the default reward-to-go: at most 1 float32 ulp apart (the float64 values
    differ by about T 2^-53 (|G| + |V|): only a rounding boundary of the cast can separate them)."""
    off, one = _rollout(case, None), _rollout(case, 1.0)
    for name in ("cross", "wait"):
        b0, b1 = getattr(off.rollout, name), getattr(one.rollout, name)
        _same(b0, b1, REC)
        if b0["ret"].numel():
            assert float(_ulp_apart(b0["ret"], b1["ret"]).max()) <= 1.0, name


@pytest.mark.parametrize("case", list(STACK))
def test_torch_path_agrees_with_native(case):
    from mhppo.rollout import bucket_segments, bucket_segments_torch
    algo = _rollout(case, 0.95)
    gamma, lam = 0.99, 0.95
    gae = (algo.critic_net_cross, algo.critic_net_wait, gamma, lam)
    batch = algo.rollout.batch
    nat = bucket_segments(batch, gae=gae)
    tor = bucket_segments_torch(batch, gae=gae)
    for k, name in enumerate(("cross", "wait")):
        a, b = nat[k], tor[k]
        assert a["n_seg"] == b["n_seg"]
        _same(a, b, REC)  # the positions and every field but ret
        if a["n_seg"] == 0:
            continue
        # ret: the two paths differ in V alone, torch's GEMM forward against forward_rows' fmaf
        # chains.  R_t = sum_k (gamma lam)^k (r_{t+k} + gamma (1 - lam) V_{t+k+1}), so values dv
        # apart move a target by at most gamma (1 - lam) dv / (1 - gamma lam) <= dv / (1 - gamma lam);
        # each path then rounds its target to float32 once (half an ulp of |ret| each).
        with torch.no_grad():
            dv = float((gae[k](a["obs"]).reshape(-1) - gae[k].forward_rows(a["obs"])).abs().max())
        ulp = float(np.spacing(np.float32(a["ret"].abs().max().item())))
        tol = dv / (1.0 - gamma * lam) + ulp
        diff = float((a["ret"] - b["ret"]).abs().max())
        print(f"{case} {name}: max |critic(obs) - forward_rows| {dv:.3g}, tolerance {tol:.3g}, max |ret diff| {diff:.3g}")
        assert dv < 1e-4  # float32 forward noise, not another function
        # measured on an MI355X (dv, tolerance, max |ret difference|):
        #   coop 2/1/2      cross 9.54e-07, 3.13e-05, 1.53e-05   wait 4.77e-07, 6.90e-05, 0
        #   scalable 8/1/4  cross 7.60e-07, 2.80e-05, 1.53e-05   wait 1.67e-06, 8.91e-05, 6.10e-05
        # every difference seen is one float32 ulp of the target (2^-16 at |ret| ~ 200, 2^-14 at
        # ~ 800): the rounding term, not the dv term, is what the paths use up
        assert diff <= tol, name
    _same(nat[2], tor[2], ("obs", "act", "logp", "ret", "counts"))


def _train(n, **kw):
    algo = _algo("coop_2_1_2", **kw)
    algo.train(n)
    torch.cuda.synchronize()
    return algo


def test_algo_trains_with_gae_lambda():
    base = _train(2)
    a = _train(2, gae_lambda=0.95)
    b = _train(2, gae_lambda=0.95)
    assert a.rollout.gae is not None and base.rollout.gae is None
    for net in a.nets():
        assert bool(torch.isfinite(net.flat()).all())
    for x, y in zip(a.nets(), b.nets()):  # the same seed twice: byte-identical nets
        assert torch.equal(x.flat(), y.flat())
    assert a.curves() == b.curves()
    # the continuous heads that trained (a non-empty bucket in the first iteration, which is the
    # same episode in both runs) trained on other targets than the default run's
    assert a.ep_scenario_balance[0] == base.ep_scenario_balance[0] and sum(a.ep_scenario_balance[0]) > 0
    for head, m in zip(("cross", "wait"), a.ep_scenario_balance[0]):
        for kind in ("actor", "critic"):
            if m:
                assert not torch.equal(getattr(a, f"{kind}_net_{head}").flat(),
                                       getattr(base, f"{kind}_net_{head}").flat()), (kind, head)
    # the choice head keeps its episodic-min target; its batch follows the continuous actors
    # only through the next rollout, so its first update is the default run's
    a1, b1 = _train(1, gae_lambda=0.95), _train(1)
    assert torch.equal(a1.actor_net_choice.flat(), b1.actor_net_choice.flat())
    assert torch.equal(a1.critic_net_choice.flat(), b1.critic_net_choice.flat())


def test_knob_off_never_reaches_the_kernel(monkeypatch):
    from mhppo import _lib
    from mhppo.rollout import returns_scan
    calls = []
    real = _lib.gae_tm
    monkeypatch.setattr(_lib, "gae_tm", lambda *a: (calls.append(1), real(*a))[1])
    algo = _algo("coop_2_1_2")
    assert algo.gae_lambda is None
    checked = []
    update = algo.update

    def spy():
        r = algo.rollout
        T = r.batch.T
        for b in (r.cross, r.wait):
            n = b["n_seg"]
            if n:
                assert torch.equal(returns_scan(b["rew"].reshape(n, T), 0.99).reshape(-1), b["ret"])
                checked.append(n)
        return update()

    algo.update = spy
    algo.train(2)
    torch.cuda.synchronize()
    assert calls == [] and checked
    on = _algo("coop_2_1_2", gae_lambda=0.95)
    on.train(2)
    assert len(calls) == 2  # one launch per iteration
