"""Early episode ends on the GPU (mhppo_record_step_done, mhppo_ragged_plan, mhppo_returns_scan_tm_len,
mhppo_gae_tm_len, mhppo_bucket_scatter_ragged; ExternalRollout(early_end=True), Algo_PPO.train_external(
early_end=True)).  Every comparison is bit for bit except the reward sums against a torch sum, which have
the bound of two summation orders.  The simulator's done comes from a host-known schedule (ScheduledSim),
never from when the env happens to end:
  1. record_step_done against record_step_done_torch, between guards, in both layouts;
  2. ragged_plan against ragged_plan_torch past one block of each launch;
  3. returns_scan_tm_len and gae_tm_len against their torch specifications; len_rec NULL = the old calls;
  4. bucket_scatter_ragged against an index-op restatement, every unowned row keeping its sentinel;
  5. ExternalRollout(early_end=True) on a VecCrosswalk: native = specification, a never-done schedule = the
     fixed-length path, the truncation property, batch() at k < T, check_every;
  6. train_external(early_end=True) against the same iterations made by hand on the torch bucketing;
  7. misuse of the Python API and of the ABI."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_external_gpu import BATCH_KEYS, TM_KEYS, algo_state, make_env, synthetic
from test_policy_gpu import guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu
SENT = -77.0
KEYS = ("obs", "act", "logp", "ret", "rew")
GAMMA = 0.99


def eq(a, b):
    return same_bits(a.cpu().numpy(), b.cpu().numpy())


def cu(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


# ------------------------------------------------------------------ the done schedule
def schedule(M, T, never=False):
    """(lengths [M], 0 = never ends; done bool [T, M]): stream r ends at 1 + (7 r) mod T, every fifth stream
    never; after its end a stream raises done again whenever (t + r) % 3 == 0."""
    r = np.arange(M)
    L = np.where(r % 5 == 4, 0, 1 + (7 * r) % T)
    if never:
        L = np.zeros(M, dtype=np.int64)
    t = np.arange(T)[:, None]
    done = (L[None, :] > 0) & ((t == L[None, :] - 1) | ((t >= L[None, :]) & ((t + r[None, :]) % 3 == 0)))
    return L, done


def check_schedule(L, done, T):
    """what the tests rely on the schedule to contain"""
    assert (L == 1).any() and (L == 0).any()
    full = np.nonzero(L == T)[0]
    assert full.size and done[T - 1, full].all() and not done[:T - 1, full].any()  # length T by a done at T - 1
    ended = np.nonzero((L > 0) & (L < T))[0]
    assert any(done[L[r]:, r].any() for r in ended)  # a done repeated after the end
    for r in np.nonzero(L > 0)[0]:
        assert done[L[r] - 1, r] and not done[:L[r] - 1, r].any()
    assert not done[:, L == 0].any()


class ScheduledSim:
    """A VecCrosswalk whose done is the schedule's (the env's own is recorded in `env_done`, and OR-ed in only
    with or_env).  The env is stepped for every stream at every step, finished or not.  reset() gives the
    episode's first rows and starts the schedule again; rew_light of every step is kept."""

    def __init__(self, env, done, or_env=False):
        self.env, self.or_env = env, or_env
        self.done = torch.from_numpy(done).cuda()
        self.t, self.rl, self.env_done = 0, [], []

    def reset(self):
        self.t, self.rl, self.env_done = 0, [], []
        return self.env.reset()

    def step(self, actions):
        obs, rew, rl, d = self.env.step(actions)
        self.rl.append(rl.clone())
        self.env_done.append(d.clone())
        done = self.done[self.t] | d if self.or_env else self.done[self.t].clone()
        self.t += 1
        return obs, rew, rl, done


# ------------------------------------------------------------------ 1. record_step_done vs spec
@pytest.mark.parametrize("compact", [False, True], ids=["identity", "compact"])
@pytest.mark.parametrize("M,S", [(1, 1), (3, 2), (257, 3), (1031, 8)])
def test_record_step_done_equals_spec(M, S, compact):
    from mhppo import _lib
    from mhppo.external import record_begin_torch, record_step_done_torch
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    T, NS = 5, M * S
    lens, done = schedule(M, T)
    if M >= 25:
        check_schedule(lens, done, T)
    if (M, S) == (257, 3):  # stream 85's segments 255, 256, 257 straddle the 256-segment block boundary
        assert 85 * S <= 255 and 256 <= 85 * S + S - 1 and 0 < lens[85] < T
    exist, steps = synthetic(M, S, 100 * M + S)
    spec = dict(obs=(T * NS * 13, torch.float32), act=(T * NS, torch.float32), logp=(T * NS, torch.float32),
                rew=(T * NS, torch.float64), ep_min=(NS, torch.float64), rec=(NS + M + 1, torch.int32), len=(M, torch.int32))
    bufs = {k: guarded(n, dt, int(SENT) if dt == torch.int32 else SENT) for k, (n, dt) in spec.items()}
    nat = {k: v[1] for k, v in bufs.items()}
    work = torch.empty(max(1, int(L.mhppo_record_work_bytes(M, S)) // 8), dtype=torch.float64, device="cuda")
    assert L.mhppo_record_begin(p(exist), M, S, p(nat["rec"]) if compact else None, p(nat["ep_min"]), p(work), st) == 0
    nat["len"].zero_()
    ep_ref, rec_ref = record_begin_torch(exist, compact)
    len_ref = torch.zeros(M, dtype=torch.int32, device="cuda")
    rec_of = nat["rec"][:NS] if compact else None
    ref = dict(obs=torch.full((T, NS, 13), SENT, device="cuda"), act=torch.full((T, NS), SENT, device="cuda"),
               logp=torch.full((T, NS), SENT, device="cuda"),
               rew=torch.full((T, NS), SENT, dtype=torch.float64, device="cuda"))
    frozen = {}  # stream -> ep_min row at its end
    for t in range(T):
        x = steps[t % len(steps)]
        rl = x["rew_light"] - 0.25 * t  # falls with t: a frozen minimum differs from a running one
        d = cu(done[t]).to(torch.uint8)
        assert L.mhppo_record_step_done(M, S, t, T, p(x["act"]), p(x["logp"]), p(x["feat_c"]), p(x["rew"]), p(rl),
                                        p(rec_of), p(nat["obs"]), p(nat["act"]), p(nat["logp"]), p(nat["rew"]),
                                        p(nat["ep_min"]), p(d), p(nat["len"]), st) == 0
        record_step_done_torch(t, x["act"], x["logp"], x["feat_c"], x["rew"], rl,
                               None if rec_of is None else rec_ref[:NS], ref["obs"], ref["act"], ref["logp"], ref["rew"],
                               ep_ref, d, len_ref)
        torch.cuda.synchronize()
        for k in ("obs", "act", "logp", "rew"):
            assert eq(nat[k], ref[k].reshape(-1)), (t, k)
        assert eq(nat["ep_min"].view(M, S), ep_ref), t
        assert eq(nat["len"], len_ref), t
        got = nat["ep_min"].view(M, S).cpu().numpy()
        for r in np.nonzero(lens == t + 1)[0]:
            frozen[int(r)] = got[r].copy()
        for r, row in frozen.items():
            assert same_bits(got[r], row), (t, r)
    assert nat["len"].tolist() == lens.tolist()  # exact: the first done, a repeated one ignored
    for k, (n, dt) in spec.items():
        assert guards_intact(bufs[k][0], n, int(SENT) if dt == torch.int32 else SENT), k
    if M >= 25:  # the running streams' minimum went on falling after the finished ones froze
        run, fin = np.nonzero(lens == 0)[0], np.nonzero(lens == 1)[0]
        e = ep_ref.cpu().numpy()
        assert np.nanmin(e[run]) < np.nanmin(e[fin])


# ------------------------------------------------------------------ 2. ragged_plan vs spec
def plan_inputs(M, S, compact, kind, seed):
    """pos / bucket per record column as mhppo_bucket_plan writes them, rec_of, len"""
    from mhppo.external import record_begin_torch
    g = torch.Generator().manual_seed(seed)
    NS = M * S
    exist = (torch.rand((M, S), generator=g) < 0.7).to(torch.uint8)
    rec_of = record_begin_torch(exist, True)[1][:NS] if compact else None
    wait = torch.rand(NS, generator=g) < 0.4
    used = exist.reshape(-1).bool() & (torch.rand(NS, generator=g) < 0.9)
    if kind == "all_cross":
        wait[:] = False
    elif kind == "all_wait":
        wait[:] = True
    elif kind == "none":
        used[:] = False
    cross, wait = used & ~wait, used & wait
    cc, cw = torch.cumsum(cross, 0), torch.cumsum(wait, 0)
    w0 = (int(cc[-1]) + 3) // 4 * 4
    pos = torch.where(cross, cc - 1, torch.where(wait, w0 + cw - 1, -1))
    bucket = wait.to(torch.int8)
    if compact:
        idx = torch.where(rec_of >= 0, rec_of, NS).long()
        pos = torch.full((NS + 1,), -1, dtype=torch.int64).scatter_(0, idx, pos)[:NS]
        bucket = torch.zeros(NS + 1, dtype=torch.int8).scatter_(0, idx, bucket)[:NS]
    return pos.cuda(), bucket.cuda(), None if rec_of is None else rec_of.cuda()


@pytest.mark.parametrize("kind", ["mixed", "all_cross", "all_wait", "none"])
@pytest.mark.parametrize("M,S,compact", [(70001, 1, False), (23000, 3, True), (5, 2, False), (300, 3, True)],
                         ids=["70001x1", "23000x3_compact", "5x2", "300x3_compact"])
def test_ragged_plan_equals_spec(M, S, compact, kind):
    from mhppo import _lib
    from mhppo.rollout import ragged_plan_torch
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    NS, T = M * S, 20
    if M > 20000:
        assert NS > 256 * 256  # more than one tile of the one-block scan, and many count / place blocks
    k = 13
    lens, _ = schedule(M, T)  # lengths up to 20 > k: they count as still running
    ln = cu(lens, torch.int32)
    pos, bucket, rec_of = plan_inputs(M, S, compact, kind, 2)  # a seed whose mixed case has rows_cross % 4 != 0
    r0b, row0 = guarded(NS, torch.int64, int(SENT))
    lrb, len_rec = guarded(NS, torch.int32, int(SENT))
    inb, info = guarded(2, torch.int64, int(SENT))
    nw = int(L.mhppo_ragged_work_bytes(NS))
    assert nw % 8 == 0 and nw >= 8
    wb, work = guarded(nw // 8, torch.int64, int(SENT))
    assert L.mhppo_ragged_plan(p(pos), p(bucket), p(rec_of), p(ln), M, S, k, p(row0), p(len_rec), p(info), p(work), st) == 0
    torch.cuda.synchronize()
    w_row0, w_len, w_info = ragged_plan_torch(pos, bucket, rec_of, ln, M, S, k)
    assert eq(row0, w_row0) and eq(len_rec, w_len) and eq(info, w_info)
    assert guards_intact(r0b, NS, int(SENT)) and guards_intact(lrb, NS, int(SENT)) and guards_intact(inb, 2, int(SENT))
    assert guards_intact(wb, nw // 8, int(SENT))
    rows_cross, rows_wait = info.tolist()
    if kind == "mixed":
        assert rows_cross % 4 != 0 and rows_wait > 0, "choose another seed: the pad rows are not exercised"
        assert int(row0[(pos >= 0) & (bucket != 0)].min()) == (rows_cross + 3) // 4 * 4
    assert (rows_cross == 0) == (kind in ("all_wait", "none")) and (rows_wait == 0) == (kind in ("all_cross", "none"))
    assert int(len_rec.max()) == k and int(len_rec[len_rec > 0].min()) == 1
    assert bool((len_rec == 0).any()) == compact
    # the same call gives the same bits
    row0_1 = row0.clone()
    assert L.mhppo_ragged_plan(p(pos), p(bucket), p(rec_of), p(ln), M, S, k, p(row0), p(len_rec), p(info), p(work), st) == 0
    torch.cuda.synchronize()
    assert eq(row0, row0_1)


# ------------------------------------------------------------------ 3. the two scans
def scan_lengths(B, T, seed):
    """(len_rec int32 [B], used bool [B]): 1 and T among the used columns, 0 on the unused ones"""
    rng = np.random.default_rng(seed)
    used = rng.random(B) >= 0.25
    used[0] = True
    ln = rng.integers(1, T + 1, B)
    ln[0] = T
    if B > 2:
        used[1:3] = True
        ln[1] = 1
    ln = np.where(used, ln, 0)
    return ln.astype(np.int32), used


@functools.lru_cache(maxsize=None)
def critics():
    from mhppo.models import Model_PPO
    torch.manual_seed(21)
    return Model_PPO(13, 1, 0).cuda(), Model_PPO(13, 1, 0).cuda()


@pytest.mark.parametrize("T", (1, 7, 19))
@pytest.mark.parametrize("B", (1, 33, 100))
def test_scans_with_lengths_equal_spec(B, T):
    from mhppo import _lib
    from mhppo.rollout import gae_targets_tm, gae_targets_torch, returns_scan_tm
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    g = torch.Generator().manual_seed(B * 100 + T)
    rew_h = torch.randn((T, B), generator=g, dtype=torch.float64)
    X = torch.randn((T, B, 13), generator=g).cuda()
    ln_h, used_h = scan_lengths(B, T, B + T)
    assert ln_h.max() == T and (B < 3 or (ln_h == 1).any()) and (B < 100 or (ln_h[~used_h] == 0).all() and not used_h.all())
    ln, rew = cu(ln_h), rew_h.cuda()
    dead = torch.arange(T)[:, None] >= torch.from_numpy(ln_h.astype(np.int64))[None, :]
    rew_nan = rew_h.clone()
    rew_nan[dead] = float("nan")  # nothing at or past a length is read into a result
    # the reward-to-go: the CPU form of returns_scan_tm is the specification
    got = returns_scan_tm(rew_nan.cuda(), GAMMA, len_rec=ln)
    assert eq(got, returns_scan_tm(rew_h, GAMMA, len_rec=torch.from_numpy(ln_h)))
    assert not bool(got.cpu()[dead].any())
    out = torch.full((T, B), SENT, dtype=torch.float32, device="cuda")
    assert L.mhppo_returns_scan_tm_len(p(rew), p(out), B, T, GAMMA, None, st) == 0
    assert eq(out, returns_scan_tm(rew, GAMMA))
    # GAE: V from the entry point without lengths; the recurrence from gae_targets_torch
    c0, c1 = critics()
    for with_pos in (True, False):
        used = cu(used_h) if with_pos else torch.ones(B, dtype=torch.bool, device="cuda")
        pos = torch.where(used, torch.cumsum(used, 0) - 1, -1) if with_pos else None
        bucket = cu(np.arange(B) % 3 == 1).to(torch.int8) if with_pos else None
        ln_u = ln if with_pos else torch.clamp(ln, min=1)  # without pos every record is used
        full, val_full = gae_targets_tm(X, rew, c0, c1 if with_pos else None, pos, bucket, GAMMA, 0.95, want_value=True)
        live = used[None, :] & (torch.arange(T, device="cuda")[:, None] < ln_u[None, :])
        Xn = X.clone()
        Xn[~live] = float("nan")
        rn = torch.where(live, rew, torch.full_like(rew, float("nan")))
        ret, val = gae_targets_tm(Xn, rn, c0, c1 if with_pos else None, pos, bucket, GAMMA, 0.95, want_value=True,
                                  len_rec=ln_u)
        assert eq(val, torch.where(live, val_full, torch.zeros_like(val_full))), with_pos
        want = gae_targets_torch(rew, val_full, GAMMA, 0.95, len_rec=torch.where(used, ln_u, torch.zeros_like(ln_u)))
        assert eq(ret, want), with_pos
        assert not bool(ret[~live].any()) and bool(ret[live].any())
        # len_rec NULL: the old entry point's bits
        r2 = torch.full((T, B), SENT, dtype=torch.float32, device="cuda")
        v2 = torch.full((T, B), SENT, dtype=torch.float32, device="cuda")
        d0, k0 = c0.mlp_desc()
        d1, k1 = c1.mlp_desc()
        assert L.mhppo_gae_tm_len(ctypes.byref(d0), ctypes.byref(d1) if with_pos else None, p(X), p(rew), p(pos), p(bucket),
                                  B, T, GAMMA, 0.95, p(r2), p(v2), None, st) == 0
        assert eq(r2, full) and eq(v2, val_full)


# ------------------------------------------------------------------ 4. bucket_scatter_ragged vs spec
def test_bucket_scatter_ragged_equals_spec():
    from mhppo import _lib
    from mhppo.rollout import ragged_plan_torch
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    NS, T, S = 130, 19, 1  # three segment tiles of 64, two step tiles of 16 (16 + 3)
    g = torch.Generator().manual_seed(9)
    lens = torch.randint(1, T + 1, (NS,), generator=g, dtype=torch.int32)
    lens[:6] = torch.tensor([1, 16, 17, 19, 1, 19], dtype=torch.int32)
    lens[63:66] = torch.tensor([16, 17, 1], dtype=torch.int32)  # across a segment-tile boundary
    used = torch.rand(NS, generator=g) < 0.85
    used[:6] = True
    wait = torch.rand(NS, generator=g) < 0.5
    cross, wait = used & ~wait, used & wait
    cc, cw = torch.cumsum(cross, 0), torch.cumsum(wait, 0)
    pos = torch.where(cross, cc - 1, torch.where(wait, (int(cc[-1]) + 3) // 4 * 4 + cw - 1, -1))
    row0, len_rec, info = ragged_plan_torch(pos, wait.to(torch.int8), None, lens, NS, S, T)
    rows_cross, rows_wait = info.tolist()
    w0 = (rows_cross + 3) // 4 * 4
    assert rows_cross % 4 != 0 and w0 > rows_cross  # pad rows between the buckets
    for v in (1, 16, 17, 19):
        assert bool((len_rec[used] == v).any())
    src = dict(obs=torch.randn((T, NS, 13), generator=g), act=torch.randn((T, NS), generator=g),
               logp=torch.randn((T, NS), generator=g), ret=torch.randn((T, NS), generator=g),
               rew=torch.randn((T, NS), generator=g, dtype=torch.float64))
    n = NS * T + 3
    tt = torch.arange(T)[:, None]
    own = (row0 >= 0)[None, :] & (tt < len_rec[None, :])
    rows = (row0[None, :] + tt)[own]
    assert rows.unique().numel() == rows.numel() == rows_cross + rows_wait and int(rows.max()) == w0 + rows_wait - 1
    want, bufs = {}, {}
    for k, x in src.items():
        w = 13 if k == "obs" else 1
        want[k] = torch.full((n, w), SENT, dtype=x.dtype)
        want[k][rows] = x.reshape(T, NS, w)[own]
        bufs[k] = guarded(n * w, x.dtype, SENT)
    one = _lib.BucketDst(*[bufs[k][1].data_ptr() for k in KEYS])
    dst = (_lib.BucketDst * 2)(one, one)
    dev = {k: v.cuda() for k, v in src.items()}
    d_row0, d_len, d_bucket = row0.cuda(), len_rec.cuda(), wait.to(torch.int8).cuda()
    work = torch.empty(max(1, int(L.mhppo_bucket_work_bytes(NS, T)) // 8), dtype=torch.float64, device="cuda")
    sums = []
    for _ in range(2):
        s = torch.zeros(2, dtype=torch.float64, device="cuda")
        assert L.mhppo_bucket_scatter_ragged(p(d_row0), p(d_bucket), p(d_len), NS, T, *[p(dev[k]) for k in KEYS], dst,
                                             p(s), p(work), st) == 0
        torch.cuda.synchronize()
        sums.append(s.cpu())
    for k in KEYS:  # the whole buffers: the pad rows between the buckets and the tail keep their sentinel
        assert eq(bufs[k][1], want[k].reshape(-1)), k
        assert guards_intact(bufs[k][0], want[k].numel(), SENT), k
        assert bool((want[k][rows_cross:w0] == SENT).all()) and bool((want[k][w0 + rows_wait:] == SENT).all())
    assert same_bits(sums[0].numpy(), sums[1].numpy())
    r32 = src["rew"].float().double()
    for b, m in enumerate((cross, wait)):
        x = r32[own & m[None, :]]
        bound = 2 * (x.numel() - 1) * 2.0 ** -53 * float(x.abs().sum())
        err = abs(float(sums[0][b]) - float(x.sum()))
        print(f"bucket {b}: n {x.numel()} |sum diff| {err:.3g} bound {bound:.3g}")
        assert err <= bound, b


# ------------------------------------------------------------------ 5. ExternalRollout(early_end=True)
ROLL = [("coop", 4, 2, 2, 0, 20), ("scalable", 4, 3, 2, 0, 20)]
N, SEED, ITER = 64, 4, 2


def roll_actors(dc):
    from test_external_gpu import actors
    return actors(dc)


@functools.lru_cache(maxsize=None)
def runs(case):
    """Once per case: the scheduled run on the native pass and on its specification, the never-done run, and
    the early_end=False run, each with its buckets."""
    from mhppo.external import ExternalRollout
    from mhppo.policy import Policy
    from mhppo.rollout import RolloutGPU, bucket_segments, bucket_segments_ragged_torch
    T = case[5]
    lens, done = schedule(N, T)
    check_schedule(lens, done, T)
    venv = make_env(case)
    ac, aw, ad = roll_actors(RolloutGPU(venv).dc)
    pol = Policy.from_env(venv, ac, aw, ad)
    out = dict(lens=lens, done=done, pol=pol)

    def run(name, early_end, native, d, bucketing):
        ext = ExternalRollout(pol, N, T=T, seed=SEED, native=native, early_end=early_end)
        sim = ScheduledSim(make_env(case), d)
        b = ext.collect(sim, ITER)
        out[name] = dict(ext=ext, sim=sim, batch=b, buckets=bucketing(b, status=ext.status))

    never = schedule(N, T, never=True)[1]
    run("sched", True, True, done, bucket_segments)
    run("spec", True, False, done, bucket_segments_ragged_torch)
    run("never", True, True, never, bucket_segments)
    run("fixed", False, True, never, bucket_segments)
    return out


def buckets_equal(x, y):
    for name, a, b in zip(("cross", "wait", "choice"), x, y):
        assert set(a) == set(b), name
        for k in a:
            if k in ("n_seg", "rows"):
                assert a[k] == b[k], (name, k)
            else:
                assert eq(a[k], b[k]), (name, k)


@pytest.mark.parametrize("case", ROLL, ids=lambda c: c[0])
def test_native_equals_spec_on_an_env(case):
    R = runs(case)
    a, b = R["sched"], R["spec"]
    assert a["batch"].steps == b["batch"].steps == case[5] and (a["batch"].rec_of is not None) == (case[0] == "scalable")
    for k in BATCH_KEYS + TM_KEYS + ("len",):
        assert eq(getattr(a["batch"], k), getattr(b["batch"], k)), k
    assert a["batch"].len.tolist() == R["lens"].tolist()
    assert a["buckets"][0]["rows"] > 0 and a["buckets"][1]["rows"] > 0
    buckets_equal(a["buckets"], b["buckets"])  # rew_sums too: the specification restates the fold's order
    # the reward sums against torch's sum of the same rows
    for i in range(2):
        x = a["buckets"][i]["rew"].float().double()
        bound = 2 * (x.numel() - 1) * 2.0 ** -53 * float(x.abs().sum())
        for who in (a, b):
            assert abs(float(who["buckets"][2]["rew_sums"][i]) - float(x.sum())) <= bound, i
    x = a["buckets"][2]["ret"].double()
    for who in (a, b):
        assert abs(float(who["buckets"][2]["rew_sums"][2]) - float(x.sum())) <= 2 * (x.numel() - 1) * 2.0 ** -53 * float(
            x.abs().sum())


@pytest.mark.parametrize("case", ROLL, ids=lambda c: c[0])
def test_never_done_is_the_fixed_length_path(case):
    R = runs(case)
    a, f = R["never"], R["fixed"]
    assert a["batch"].len.tolist() == [0] * N
    T = case[5]
    for name, x, y in zip(("cross", "wait", "choice"), a["buckets"], f["buckets"]):
        assert set(x) - set(y) <= {"rows"} and set(y) <= set(x), name
        for k in y:
            if k == "n_seg":
                assert x[k] == y[k], (name, k)
            else:
                assert eq(x[k], y[k]), (name, k)
    assert a["buckets"][0]["rows"] == f["buckets"][0]["n_seg"] * T and a["buckets"][1]["rows"] == f["buckets"][1]["n_seg"] * T


def truncated(R, case, got, lens_eff, rl_steps):
    """The truncation property of buckets `got` against the never-done run, for effective lengths lens_eff [N]."""
    from mhppo.rollout import bucket_segments_torch
    T = case[5]
    nb = R["never"]["batch"]
    S = nb.S
    plan = {}
    bucket_segments_torch(nb, plan_out=plan)
    exist = nb.exist.reshape(-1).bool().cpu()
    wait = plan["wait"].cpu()
    seg_len = torch.from_numpy(np.repeat(lens_eff, S))
    total = 0
    for i, mask in enumerate((exist & ~wait, exist & wait)):
        full, g = R["never"]["buckets"][i], got[i]
        Ls = seg_len[mask]
        assert full["n_seg"] == g["n_seg"] == int(mask.sum()) and g["rows"] == int(Ls.sum()) == g["act"].numel()
        total += g["rows"]
        keep = torch.arange(T)[None, :] < Ls[:, None]  # [n_seg, T]
        for k in ("obs", "act", "logp", "rew"):
            x = full[k].cpu().reshape(full["n_seg"], T, -1)[keep]
            assert same_bits(g[k].cpu().reshape(x.shape).numpy(), x.numpy()), (i, k)
        # ret: the float64 recomputation on the truncated rewards
        rew = full["rew"].cpu().reshape(full["n_seg"], T).numpy()
        want = []
        for j, Lj in enumerate(Ls.tolist()):
            G, r = 0.0, np.zeros(Lj, dtype=np.float32)
            for t in range(Lj - 1, -1, -1):
                G = rew[j, t] + GAMMA * G
                r[t] = np.float32(G)
            want.append(r)
        assert same_bits(g["ret"].cpu().numpy(), np.concatenate(want)), i
    assert total == int(seg_len[exist].sum())
    # the choice ret: the NaN-propagating minimum of reward_light over the first L steps
    m = torch.zeros_like(rl_steps[0]).cpu()
    for t, x in enumerate(rl_steps):
        x = x.cpu()
        new = torch.where(m != m, m, torch.where(x != x, x, torch.where(x < m, x, m)))
        m = torch.where(torch.from_numpy(lens_eff > t)[:, None], new, m)
    assert same_bits(got[2]["ret"].cpu().numpy(), m.reshape(-1)[exist].float().numpy())
    assert got[2]["n_seg"] == int(exist.sum())


@pytest.mark.parametrize("case", ROLL, ids=lambda c: c[0])
def test_truncation_property(case):
    R = runs(case)
    T = case[5]
    lens_eff = np.where(R["lens"] > 0, R["lens"], T)
    assert (lens_eff < T).any()
    truncated(R, case, R["sched"]["buckets"], lens_eff, R["sched"]["sim"].rl)
    # the scheduled run's reward_light rows are the never-done run's: the same sim, the same draws
    for x, y in zip(R["sched"]["sim"].rl, R["never"]["sim"].rl):
        assert eq(x, y)
    full, cut = R["never"]["buckets"][2]["ret"], R["sched"]["buckets"][2]["ret"]
    assert not eq(full, cut)  # the episodic minimum did go on falling after some end


@pytest.mark.parametrize("case", ROLL, ids=lambda c: c[0])
def test_batch_before_T_cuts_the_running_streams(case):
    from mhppo.external import ExternalRollout
    from mhppo.rollout import bucket_segments
    R = runs(case)
    T, k = case[5], 7
    ext = ExternalRollout(R["pol"], N, T=T, seed=SEED, early_end=True)
    sim = ScheduledSim(make_env(case), R["done"])
    obs = sim.reset()
    ext.begin(obs, ITER)
    for t in range(k):
        obs, rew, rl, d = sim.step(ext.act(obs, t))
        ext.record(rew, rl, d)
    b = ext.batch()
    assert b.steps == k and b.T == T
    lens_eff = np.where((R["lens"] > 0) & (R["lens"] <= k), R["lens"], k)
    assert b.len.tolist() == np.where(R["lens"] <= k, R["lens"], 0).tolist() and (lens_eff == k).sum() > (R["lens"] == k).sum()
    truncated(R, case, bucket_segments(b, status=ext.status), lens_eff, sim.rl)


def test_check_every_stops_after_the_last_end():
    from mhppo.external import ExternalRollout
    case = ROLL[0]
    R = runs(case)
    T = case[5]
    lens = 1 + (7 * np.arange(N)) % 9  # every stream ends, the last at step 9
    assert lens.max() == 9
    done = np.arange(T)[:, None] == lens[None, :] - 1
    ext = ExternalRollout(R["pol"], N, T=T, seed=SEED, early_end=True)
    sim = ScheduledSim(make_env(case), done)
    b = ext.collect(sim, ITER, check_every=4)
    assert b.steps == 12 == sim.t and b.len.tolist() == lens.tolist()  # the first check at or after step 9
    sim = ScheduledSim(make_env(case), done)
    assert ext.collect(sim, ITER).steps == T == sim.t  # no host read: T steps
    sim = ScheduledSim(make_env(case), R["done"])
    assert ext.collect(sim, ITER, check_every=1).steps == T  # a stream that never ends: T steps


def test_env_done_is_taken_when_ored_in():
    """the env's own done, OR-ed over the schedule: len is the first done the wrapper returned, whenever that was"""
    from mhppo.external import ExternalRollout
    case = ROLL[0]
    R = runs(case)
    T = case[5]
    ext = ExternalRollout(R["pol"], N, T=T, seed=SEED, early_end=True)
    sim = ScheduledSim(make_env(case), R["done"], or_env=True)
    b = ext.collect(sim, ITER)
    seen = torch.stack(sim.env_done).cpu().numpy() | R["done"]
    first = np.where(seen.any(0), seen.argmax(0) + 1, 0)
    assert b.len.tolist() == first.tolist()


# ------------------------------------------------------------------ 6. training
@pytest.mark.parametrize("opts", [{}, dict(gae_lambda=0.95), dict(minibatches=2, max_grad_norm=0.5)],
                         ids=["plain", "gae", "minibatch_clip"])
def test_train_external_early_end_equals_by_hand(opts):
    from mhppo.algo import Algo_PPO
    from mhppo.external import ExternalRollout
    from mhppo.models import Model_PPO
    from mhppo.rollout import bucket_segments_ragged_torch
    case = ("scalable", 4, 3, 2, 0, 20)
    T = case[5]
    lens, done = schedule(N, T)
    torch.manual_seed(3)
    a = Algo_PPO(Model_PPO, make_env(case), seed=6, verbose=False, save_curves=False, **opts)
    b = Algo_PPO(Model_PPO, make_env(case), seed=6, verbose=False, save_curves=False, **opts)
    for na, nb in zip(a.nets(), b.nets()):
        nb.load_state_dict(na.state_dict())
    before = {k: v.clone() for k, v in algo_state(a).items()}
    sim_a, sim_b = ScheduledSim(make_env(case), done), ScheduledSim(make_env(case), done)
    a.train_external(sim_a, 2, M=N, early_end=True)
    assert a._external[0] == (N, T, True) and a.rollout.batch.len.tolist() == lens.tolist()
    assert a.rollout.cross["rows"] + a.rollout.wait["rows"] < (a.rollout.cross["n_seg"] + a.rollout.wait["n_seg"]) * T
    # the same two iterations by hand, on the torch specification of the bucketing
    r = b.rollout
    r.fix_bucket = b.fix_bucket
    lam = getattr(b, "gae_lambda", None)
    r.gae = None if lam is None else (b.critic_net_cross, b.critic_net_wait, b.gamma, lam)
    ext = ExternalRollout(b.policy(), N, T=T, early_end=True)
    ext.session.first_env = int(b.venv.cfg.env_id_offset)
    for ep in range(2):
        ext.session.seed = int(r.seed)
        r.batch = ext.collect(sim_b, r.iteration)
        r.iteration += 1
        r.cross, r.wait, r.choice = bucket_segments_ragged_torch(r.batch, fix_bucket=r.fix_bucket, status=ext.status,
                                                                 gae=r.gae)
        b._after_collect(ep, reset_env=False)
    b._finish_train()
    sa, sb = algo_state(a), algo_state(b)
    assert set(sa) == set(sb) and any(k.startswith("opt.") and k.endswith("exp_avg") for k in sa)
    for k in sa:
        assert eq(sa[k], sb[k]), k
    assert any(not eq(sa[k], before[k]) for k in before if k.startswith("net"))
    ca, cb = a.curves(), b.curves()
    print("curves", ca, cb)
    assert ca == cb and len(ca[2]) == 2
    assert a.rollout.iteration == b.rollout.iteration == 2 and a.total_loop == b.total_loop == 2
    # early_end is part of the cache key: the fixed-length rollout is another object
    a.train_external(ScheduledSim(make_env(case), done), 1, M=N)
    assert a._external[0] == (N, T, False) and getattr(a.rollout.batch, "len", None) is None


# ------------------------------------------------------------------ 7. misuse
def test_api_rejects_misuse():
    from mhppo.env import VecCrosswalk
    from mhppo.external import ExternalRollout
    from mhppo.policy import Policy
    from test_policy_gpu import nets
    ac, aw, ad = nets(17)
    pol = Policy("coop", 2, 1, 2, ac, aw, ad)
    M, S, T = 5, pol.n_slots, 3
    obs = VecCrosswalk("coop", M, 2, 1, 2, seed_base=3).reset()
    rew = torch.zeros((M, S), dtype=torch.float64, device="cuda")
    done = torch.zeros(M, dtype=torch.bool, device="cuda")
    fixed = ExternalRollout(pol, M, T=T)
    assert fixed.len is None
    fixed.begin(obs, 0)
    fixed.act(obs, 0)
    with pytest.raises(ValueError):
        fixed.record(rew, rew, done)  # done without early_end
    with pytest.raises(ValueError):
        fixed.collect(None, 0, check_every=2)
    fixed.record(rew, rew)
    with pytest.raises(ValueError):
        fixed.batch()  # the fixed-length batch still needs all T steps
    ext = ExternalRollout(pol, M, T=T, early_end=True)
    with pytest.raises(ValueError):
        ext.batch()  # before begin
    ext.begin(obs, 0)
    with pytest.raises(ValueError):
        ext.batch()  # no step recorded
    ext.act(obs, 0)
    for bad in (None, done[:4], done.reshape(M, 1), done.cpu(), done.float(), done.int(), [False] * M):
        with pytest.raises(ValueError):
            ext.record(rew, rew, bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            ext.collect(None, 0, check_every=bad)
    ext.record(rew, rew, done.to(torch.uint8))  # uint8 is taken as it is
    b = ext.batch()
    assert b.steps == 1 and b.len.tolist() == [0] * M
    ext.act(obs, 1)
    ext.record(rew, rew, ~done)
    assert ext.batch().len.tolist() == [2] * M
    ext.begin(obs, 1)  # a new episode: the lengths start again
    assert ext.len.tolist() == [0] * M


def test_abi_rejects_bad_input():
    from mhppo import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    M, S, T = 4, 2, 3
    NS = M * S
    f = lambda n: torch.full((n,), SENT, dtype=torch.float32, device="cuda")
    d = lambda n: torch.full((n,), SENT, dtype=torch.float64, device="cuda")
    i32 = lambda n: torch.full((n,), int(SENT), dtype=torch.int32, device="cuda")
    i64 = lambda n: torch.full((n,), int(SENT), dtype=torch.int64, device="cuda")
    src = dict(act=f(NS), logp=f(NS), feat_c=f(NS * 13), rew=d(NS), rew_light=d(NS))
    dst = dict(obs=f(T * NS * 13), act=f(T * NS), logp=f(T * NS), rew=d(T * NS), ep_min=d(NS))
    done, ln = torch.ones(M, dtype=torch.uint8, device="cuda"), i32(M)

    def step(M=M, S=S, t=0, T=T, done=done, ln=ln, **null):
        a = {**src, **{"d_" + k: v for k, v in dst.items()}}
        a = {k: (None if k in null else p(v)) for k, v in a.items()}
        return L.mhppo_record_step_done(M, S, t, T, a["act"], a["logp"], a["feat_c"], a["rew"], a["rew_light"], None,
                                        a["d_obs"], a["d_act"], a["d_logp"], a["d_rew"], a["d_ep_min"], p(done), p(ln), st)

    bad = [step(t=-1), step(t=T), step(M=-1), step(S=0), step(M=2**30, S=2), step(done=None), step(ln=None)]
    bad += [step(**{k: 1}) for k in list(src) + ["d_" + k for k in dst]]
    assert all(rc == -1 for rc in bad), bad
    assert b"record_step_done" in L.mhppo_last_error()
    # M == 0 touches nothing, whatever the pointers
    assert step(M=0) == 0 and L.mhppo_record_step_done(0, 3, 0, 1, *([None] * 13), st) == 0
    # the ragged plan
    pos, bucket, row0, lrec, info, work = i64(NS), torch.zeros(NS, dtype=torch.int8, device="cuda"), i64(NS), i32(NS), i64(2), i64(16)

    def plan(M=M, S=S, k=2, pos=pos, bucket=bucket, ln=ln, row0=row0, lrec=lrec, info=info, work=work):
        return L.mhppo_ragged_plan(p(pos), p(bucket), None, p(ln), M, S, k, p(row0), p(lrec), p(info), p(work), st)

    bad = [plan(k=0), plan(M=-1), plan(S=0), plan(M=2**30, S=2), plan(info=None), plan(work=None), plan(pos=None),
           plan(bucket=None), plan(ln=None), plan(row0=None), plan(lrec=None)]
    assert all(rc == -1 for rc in bad), bad
    assert b"ragged_plan" in L.mhppo_last_error()
    assert L.mhppo_ragged_work_bytes(0) >= 8 and L.mhppo_ragged_work_bytes(-1) == 0
    # the scans
    ret = f(T * NS)
    assert L.mhppo_returns_scan_tm_len(None, p(ret), NS, T, GAMMA, p(lrec), st) == -1
    assert L.mhppo_returns_scan_tm_len(p(dst["rew"]), None, NS, T, GAMMA, p(lrec), st) == -1
    assert L.mhppo_returns_scan_tm_len(p(dst["rew"]), p(ret), -1, T, GAMMA, p(lrec), st) == -1
    assert L.mhppo_returns_scan_tm_len(p(dst["rew"]), p(ret), NS, 0, GAMMA, p(lrec), st) == -1
    assert L.mhppo_returns_scan_tm_len(p(dst["rew"]), p(ret), 0, T, GAMMA, p(lrec), st) == 0
    c0, c1 = critics()
    d0, keep = c0.mlp_desc()
    gae = lambda T=T, obs=dst["obs"], lam=0.9: L.mhppo_gae_tm_len(ctypes.byref(d0), None, p(obs), p(dst["rew"]), None, None,
                                                                  NS, T, GAMMA, lam, p(ret), None, p(lrec), st)
    assert gae(T=0) == -1 and gae(obs=None) == -1 and gae(lam=1.5) == -1
    # the ragged scatter
    one = _lib.BucketDst(*[dst[k].data_ptr() for k in ("obs", "act", "logp", "act", "rew")])
    two = (_lib.BucketDst * 2)(one, one)
    sums = d(2)
    a = dict(row0=row0, bucket=bucket, lrec=lrec, obs=dst["obs"], act=dst["act"], logp=dst["logp"], ret=ret, rew=dst["rew"])

    def scatter(NS=NS, T=T, dst_=two, sums=sums, work=work, **null):
        q = {k: (None if k in null else p(v)) for k, v in a.items()}
        return L.mhppo_bucket_scatter_ragged(q["row0"], q["bucket"], q["lrec"], NS, T, q["obs"], q["act"], q["logp"],
                                             q["ret"], q["rew"], dst_, p(sums), p(work), st)

    bad = [scatter(NS=-1), scatter(T=0), scatter(dst_=None), scatter(sums=None), scatter(work=None)]
    bad += [scatter(**{k: 1}) for k in a]
    assert all(rc == -1 for rc in bad), bad
    assert scatter(NS=0) == 0
    torch.cuda.synchronize()
    for v in list(dst.values()) + [ln, row0, lrec, info, work, ret, sums, pos]:
        assert bool((v == (int(SENT) if v.dtype in (torch.int32, torch.int64) else SENT)).all())
