"""Auto-reset lanes on the GPU (mhppo_lanes_begin / _restart / _record / _close, mhppo_returns_scan_tm_lanes,
mhppo_bucket_scatter_lanes; ExternalRollout(auto_reset=E), Algo_PPO.train_external(auto_reset=E)).  Every
comparison is bit for bit.  The simulator's done comes from the early-end tests' host-known schedule, whose
dones after a stream's first end are further episode ends here:
  1. the four bookkeeping calls against their torch specifications, between guards;
  2. returns_scan_tm_lanes and bucket_scatter_lanes against theirs, with and without v_boot, unowned rows and
     records keeping their sentinel or zero;
  3. ExternalRollout(auto_reset=3) on a VecCrosswalk: native = specification, with exist changing between a
     stream's lanes on the scalable variant;
  4. equivalences with the code that was there: auto_reset=1 is early_end=True; a never-done schedule with any E
     is early_end=True, bootstrapped or not;
  5. a restarting stream's new decision is Policy.sample_decide on that row with the uniforms at the stated
     Philox counter; the other streams keep theirs;
  6. train_external(auto_reset=2) against the same iterations made by hand on the torch bucketing;
  7. misuse of the Python API and of the ABI."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from test_early_end_gpu import (GAMMA, ITER, ROLL, SEED, SENT, ScheduledSim, buckets_equal, critics, cu, eq, roll_actors,
                                schedule)
from test_external_gpu import TM_KEYS, algo_state, make_env, synthetic
from test_policy_gpu import guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu
T7 = 7
P2, DC = 2, 5
DEC = ("a_d", "logp_d", "probs", "feat_d", "closest", "exist")
SHAPES = [(1, 1), (3, 2), (67, 4), (257, 3)]  # 268 and 771 segments cross the 256-segment block, unaligned
N67 = 67
LANE_KEYS = ("a_d", "logp_d", "probs_d", "feat_d", "closest", "exist", "ep_min", "t0", "len", "cut")


def decisions(M, S, n, seed):
    """n random SampleDecision-like sets on the GPU"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        out.append(types.SimpleNamespace(
            a_d=(torch.rand((M, S, P2), generator=g) < 0.5).to(torch.int32).cuda(),
            logp_d=torch.randn((M, S, P2), generator=g).cuda(), probs=torch.rand((M, S, P2, 2), generator=g).cuda(),
            feat_d=torch.randn((M, S, P2, DC), generator=g).cuda(),
            closest=torch.randint(0, P2, (M, S), generator=g, dtype=torch.int32).cuda(),
            exist=(torch.rand((M, S), generator=g) < 0.7).to(torch.uint8).cuda()))
    return out


def dec_struct(d):
    from mhppo import _lib
    return _lib.Decision(*[getattr(d, k).data_ptr() for k in DEC])


def lanes_struct(a):
    from mhppo import _lib
    return _lib.Lanes(_lib.Decision(*[a[k].data_ptr() for k in DEC]), a["ep_min"].data_ptr(), a["t0"].data_ptr(),
                      a["len"].data_ptr(), a["cur"].data_ptr())


def fill_of(dt):
    return SENT if dt.is_floating_point else (77 if dt == torch.uint8 else int(SENT))


# ------------------------------------------------------------------ 1. the bookkeeping vs spec
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("M,S", SHAPES)
def test_bookkeeping_equals_spec(M, S, E):
    from mhppo import _lib
    from mhppo.external import lanes_begin_torch, lanes_close_torch, lanes_record_torch, lanes_restart_torch
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    T, NS = T7, M * S
    _, done = schedule(M, T)
    decs = decisions(M, S, T, 100 * M + S)
    _, steps = synthetic(M, S, 100 * M + S)
    # the specification's state, and the native one between guards
    cur_ref = types.SimpleNamespace(**{k: getattr(decs[0], k).clone() for k in DEC})
    ref = lanes_begin_torch(cur_ref, E)
    bufs = {k: guarded(v.numel(), v.dtype, fill_of(v.dtype)) for k, v in ref.items()}
    nat = {k: bufs[k][1] for k in ref}
    cur_b = {k: guarded(getattr(decs[0], k).numel(), getattr(decs[0], k).dtype, fill_of(getattr(decs[0], k).dtype)) for k in DEC}
    cur_nat = types.SimpleNamespace(**{k: cur_b[k][1] for k in DEC})
    for k in DEC:
        cur_nat.__dict__[k].copy_(getattr(decs[0], k).reshape(-1))
    rec_spec = dict(obs=(T * NS * 13, torch.float32), act=(T * NS, torch.float32), logp=(T * NS, torch.float32),
                    rew=(T * NS, torch.float64))
    rec_b = {k: guarded(n, dt, SENT) for k, (n, dt) in rec_spec.items()}
    rec_ref = dict(obs=torch.full((T, NS, 13), SENT, device="cuda"), act=torch.full((T, NS), SENT, device="cuda"),
                   logp=torch.full((T, NS), SENT, device="cuda"), rew=torch.full((T, NS), SENT, dtype=torch.float64, device="cuda"))
    ls = lanes_struct(nat)

    def same_state(where):
        torch.cuda.synchronize()
        for k in ref:
            assert eq(nat[k], ref[k].reshape(-1)), (where, k)
        for k in DEC:
            assert eq(getattr(cur_nat, k), getattr(cur_ref, k).reshape(-1)), (where, "current", k)

    assert L.mhppo_lanes_begin(ctypes.byref(ls), E, M, S, P2, DC, ctypes.byref(dec_struct(decs[0])), st) == 0
    same_state("begin")
    restarted = 0
    for t in range(T):
        if t >= 1:
            before = ref["t0"].clone()
            assert L.mhppo_lanes_restart(ctypes.byref(ls), E, M, S, P2, DC, t, T, ctypes.byref(dec_struct(decs[t])),
                                         ctypes.byref(dec_struct(cur_nat)), st) == 0
            lanes_restart_torch(ref, t, decs[t], cur_ref)
            same_state(("restart", t))
            restarted += int((ref["t0"] != before).sum())
        x = steps[t % len(steps)]
        rl = x["rew_light"] - 0.25 * t  # falls with t: a frozen minimum differs from a running one
        d = cu(done[t]).to(torch.uint8)
        assert L.mhppo_lanes_record(ctypes.byref(ls), E, M, S, t, T, p(x["act"]), p(x["logp"]), p(x["feat_c"]), p(x["rew"]),
                                    p(rl), *[p(rec_b[k][1]) for k in ("obs", "act", "logp", "rew")], p(d), st) == 0
        lanes_record_torch(ref, t, x["act"], x["logp"], x["feat_c"], x["rew"], rl, rec_ref["obs"], rec_ref["act"],
                           rec_ref["logp"], rec_ref["rew"], d)
        same_state(("record", t))
        for k in rec_ref:  # the whole buffers: the steps not yet recorded keep their sentinel
            assert eq(rec_b[k][1], rec_ref[k].reshape(-1)), (t, k)
        for k in (2, T):
            if t + 1 == k:  # close leaves the lanes alone: recording goes on after the one at k = 2
                lb, ln = guarded(E * M, torch.int32, int(SENT))
                cb, cut = guarded(E * M, torch.uint8, 77)
                assert L.mhppo_lanes_close(ctypes.byref(ls), E, M, k, T, p(ln), p(cut), st) == 0
                w_ln, w_cut = lanes_close_torch(ref, k)
                same_state(("close", k))
                assert eq(ln, w_ln) and eq(cut, w_cut), k
                assert guards_intact(lb, E * M, int(SENT)) and guards_intact(cb, E * M, 77)
    for k, v in ref.items():
        assert guards_intact(bufs[k][0], v.numel(), fill_of(v.dtype)), k
    for k in DEC:
        assert guards_intact(cur_b[k][0], getattr(decs[0], k).numel(), fill_of(getattr(decs[0], k).dtype)), k
    for k, (n, dt) in rec_spec.items():
        assert guards_intact(rec_b[k][0], n, SENT), k
    assert (restarted > 0) == (E > 1)
    if M >= 67:  # a stream that never ends: its lane is cut; the others' are not
        assert bool(w_cut.any()) and not bool(w_cut.all())
    if E == 1:  # one lane: the early-end lengths
        lens = np.where(done.any(0), done.argmax(0) + 1, 0)
        assert ref["len"].tolist() == lens.tolist()


# ------------------------------------------------------------------ 2. the scan and the scatter vs spec
@functools.lru_cache(maxsize=None)
def lanes_state(M, S, E):
    """A lanes batch on the GPU from the specification's bookkeeping over the schedule, with random records"""
    from mhppo.external import lanes_begin_torch, lanes_close_torch, lanes_record_torch, lanes_restart_torch
    from mhppo.rollout import RolloutBatch
    T, NS = T7, M * S
    _, done = schedule(M, T)
    decs = decisions(M, S, T, 7 * M + S)
    g = torch.Generator().manual_seed(M + S + E)
    cur = types.SimpleNamespace(**{k: getattr(decs[0], k).clone() for k in DEC})
    lanes = lanes_begin_torch(cur, E)
    recs = (torch.zeros((T, NS, 13), device="cuda"), torch.zeros((T, NS), device="cuda"), torch.zeros((T, NS), device="cuda"),
            torch.zeros((T, NS), dtype=torch.float64, device="cuda"))
    for t in range(T):
        if t >= 1:
            lanes_restart_torch(lanes, t, decs[t], cur)
        lanes_record_torch(lanes, t, torch.randn((M, S), generator=g).cuda(), torch.randn((M, S), generator=g).cuda(),
                           torch.randn((M, S, 13), generator=g).cuda(), torch.randn((M, S), generator=g, dtype=torch.float64).cuda(),
                           -torch.rand((M, S), generator=g, dtype=torch.float64).cuda(), *recs, cu(done[t]))
    ln, cut = lanes_close_torch(lanes, T)
    return RolloutBatch(feat_d=lanes["feat_d"], probs_d=lanes["probs"], logp_d=lanes["logp_d"], a_d=lanes["a_d"],
                        closest=lanes["closest"], exist=lanes["exist"], ep_min=lanes["ep_min"],
                        obs_c_tm=recs[0].reshape(T, M, S, 13), act_tm=recs[1].reshape(T, M, S), logp_tm=recs[2].reshape(T, M, S),
                        rew_tm=recs[3].reshape(T, M, S), rec_of=None, N=M, M=M, S=S, P=P2, T=T, lanes=E, t0=lanes["t0"],
                        len=ln, cut=cut, steps=T, feat_tail=None, cut_truncates=True)


@pytest.mark.parametrize("boot", [False, True], ids=["plain", "v_boot"])
@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("M,S", SHAPES)
def test_scan_and_scatter_equal_spec(M, S, E, boot):
    from mhppo import _lib
    from mhppo.rollout import _scatter_sums_sel, bucket_segments_lanes_torch, returns_scan_tm_lanes_torch
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    b = lanes_state(M, S, E)
    T, NS, NL = T7, M * S, E * M * S
    plan = {}
    cross, wait, choice = bucket_segments_lanes_torch(b, plan_out=plan)
    pos, bucket, row0 = plan["pos"], plan["bucket"], plan["row0"]
    v_boot = torch.randn(NS, generator=torch.Generator().manual_seed(M)).cuda() if boot else None
    rew = b.rew_tm.reshape(T, NS)
    want_ret = returns_scan_tm_lanes_torch(rew, M, S, E, GAMMA, pos, b.t0, b.len, b.cut, v_boot)
    if not boot:
        assert eq(want_ret, plan["ret_tm"])
    rb, ret = guarded(T * NS, torch.float32, SENT)
    assert L.mhppo_returns_scan_tm_lanes(p(rew), p(ret), M, S, E, T, GAMMA, p(pos), p(b.t0), p(b.len), p(b.cut), p(v_boot),
                                         st) == 0
    torch.cuda.synchronize()
    assert eq(ret, want_ret.reshape(-1)) and guards_intact(rb, T * NS, SENT)
    if M >= 3:
        assert bool((want_ret == 0).any()) and bool((want_ret != 0).any())  # records in no used lane are 0, not the sentinel
        if boot and M >= 67:  # a used lane is cut
            assert not eq(want_ret, plan["ret_tm"])
    # the scatter of the specification's own ret: rows outside the two buckets keep their sentinel
    n = NS * T + 3
    rows_cross, rows_wait = cross["rows"], wait["rows"]
    w0 = (rows_cross + 3) // 4 * 4
    src = dict(obs=b.obs_c_tm, act=b.act_tm, logp=b.logp_tm, ret=plan["ret_tm"], rew=b.rew_tm)
    want, bufs = {}, {}
    for k, x in src.items():
        w = 13 if k == "obs" else 1
        want[k] = torch.full((n, w), SENT, dtype=x.dtype, device="cuda")
        want[k][:rows_cross] = cross[k].reshape(rows_cross, w)
        want[k][w0:w0 + rows_wait] = wait[k].reshape(rows_wait, w)
        bufs[k] = guarded(n * w, x.dtype, SENT)
    one = _lib.BucketDst(*[bufs[k][1].data_ptr() for k in ("obs", "act", "logp", "ret", "rew")])
    dst = (_lib.BucketDst * 2)(one, one)
    nw = int(L.mhppo_bucket_work_bytes(NS, T))
    wb, work = guarded(nw // 8, torch.float64, SENT)
    sums = torch.zeros(2, dtype=torch.float64, device="cuda")
    srcs = [src[k].contiguous() for k in ("obs", "act", "logp", "ret", "rew")]
    assert L.mhppo_bucket_scatter_lanes(p(row0), p(bucket), p(b.t0), p(b.len), M, S, E, T, *[p(x) for x in srcs], dst, p(sums),
                                        p(work), st) == 0
    torch.cuda.synchronize()
    for k in src:
        assert eq(bufs[k][1], want[k].reshape(-1)), k
        assert guards_intact(bufs[k][0], want[k].numel(), SENT), k
    assert guards_intact(wb, nw // 8, SENT)
    assert eq(sums, choice["rew_sums"][:2])
    for i, x in enumerate((cross["rew"], wait["rew"])):
        x = x.float().double()
        assert abs(float(sums[i]) - float(x.sum())) <= 2 * max(0, x.numel() - 1) * 2.0 ** -53 * float(x.abs().sum()), i
    if M >= 67:
        assert rows_cross > 0 and rows_wait > 0


# ------------------------------------------------------------------ 3. ExternalRollout(auto_reset=3)
def lane_lists(done, E, k):
    """per stream the (t0, len, cut) of its lanes, from the done tape"""
    out = []
    for r in range(done.shape[1]):
        eps, t0 = [], 0
        for t in range(k):
            if t0 is None:
                if len(eps) == E:
                    break
                t0 = t
            if done[t, r]:
                eps.append((t0, t + 1 - t0, 0))
                t0 = None
        if t0 is not None:
            eps.append((t0, k - t0, 1))
        out.append(eps)
    return out


class SwapSim(ScheduledSim):
    """ScheduledSim over two differently seeded envs stepped on the same actions: a stream reads env A in its
    even episodes and env B in its odd ones, so the row after a done is another scene's -- what a resetting
    simulator hands over (on the scalable variant, with other car slots present)."""

    def __init__(self, env, env_b, done):
        super().__init__(env, done)
        self.env_b, self.on_b = env_b, None

    def reset(self):
        self.on_b = torch.zeros(self.done.shape[1], dtype=torch.bool, device="cuda")
        self.env_b.reset()
        return super().reset()

    def step(self, actions):
        oa, ra, la, done = super().step(actions)
        ob, rb, lb, _ = self.env_b.step(actions)
        b = self.on_b[:, None]
        rew, rl = torch.where(b, rb, ra), torch.where(b, lb, la)  # this step still belongs to the running episode
        self.on_b = self.on_b ^ done
        return torch.where(self.on_b[:, None], ob, oa), rew, rl, done


def env_b(case):
    from mhppo.env import VecCrosswalk
    variant, nb_car, nb_ped, nb_lines, off, T = case
    return VecCrosswalk(variant, N67, nb_car, nb_ped, nb_lines, max_episode=T, seed_base=1900, env_id_offset=off)


@functools.lru_cache(maxsize=None)
def runs(case):
    from mhppo.external import ExternalRollout
    from mhppo.policy import Policy
    from mhppo.rollout import RolloutGPU, bucket_segments, bucket_segments_lanes_torch
    T = case[5]
    lens, done = schedule(N67, T)
    venv = make_env(case, N67)
    ac, aw, ad = roll_actors(RolloutGPU(venv).dc)
    pol = Policy.from_env(venv, ac, aw, ad)
    out = dict(lens=lens, done=done, pol=pol, never=schedule(N67, T, never=True)[1])

    def run(name, d, bucketing, swap=False, **kw):
        ext = ExternalRollout(pol, N67, T=T, seed=SEED, **kw)
        sim = SwapSim(make_env(case, N67), env_b(case), d) if swap else ScheduledSim(make_env(case, N67), d)
        b = ext.collect(sim, ITER)
        boot = critics() if kw.get("bootstrap") else None
        out[name] = dict(ext=ext, sim=sim, batch=b, buckets=bucketing(b, status=ext.status, boot=boot))

    run("lanes", done, bucket_segments, swap=True, auto_reset=3)
    run("spec", done, bucket_segments_lanes_torch, swap=True, auto_reset=3, native=False)
    run("one", done, bucket_segments, auto_reset=1)
    run("early", done, bucket_segments, early_end=True)
    run("never3", out["never"], bucket_segments, auto_reset=3)
    run("never_early", out["never"], bucket_segments, early_end=True)
    return out


@pytest.mark.parametrize("case", ROLL, ids=lambda c: c[0])
def test_native_equals_spec_on_an_env(case):
    R = runs(case)
    a, b = R["lanes"], R["spec"]
    T, E = case[5], 3
    assert a["batch"].lanes == b["batch"].lanes == E and a["batch"].steps == T and a["batch"].rec_of is None
    assert a["ext"].compact is False and getattr(a["batch"], "trunc", None) is None
    for k in LANE_KEYS + TM_KEYS:
        assert eq(getattr(a["batch"], k), getattr(b["batch"], k)), k
    want = lane_lists(R["done"], E, T)
    t0, ln, cut = (getattr(a["batch"], k).reshape(E, N67).cpu().numpy() for k in ("t0", "len", "cut"))
    for r, eps in enumerate(want):
        eps = eps + [(0, 0, 0)] * (E - len(eps))
        assert [(int(t0[e, r]), int(ln[e, r]), int(cut[e, r])) for e in range(E)] == eps, r
    assert any(len(e) == E for e in want) and any(len(e) == 1 for e in want)
    ex = a["batch"].exist.reshape(E, N67, -1)
    started = torch.from_numpy(np.array([[e < len(x) for x in want] for e in range(E)])).cuda()
    assert not bool(ex[~started].any())
    if case[0] == "scalable":  # exist changes from one episode of a stream to the next
        assert bool(((ex[0] != ex[1]).any(1) & started[1]).any())
    else:
        assert bool(ex[started].all())
    assert a["buckets"][0]["rows"] > 0 and a["buckets"][1]["rows"] > 0
    buckets_equal(a["buckets"], b["buckets"])  # rew_sums too: the specification restates the fold's order
    # more rows and more choice decisions than the first-done-ends-the-stream batch of the same schedule
    e1 = R["early"]["buckets"]
    assert a["buckets"][0]["rows"] + a["buckets"][1]["rows"] > e1[0]["rows"] + e1[1]["rows"]
    assert a["buckets"][2]["n_seg"] > e1[2]["n_seg"]
    # lane 0 saw the same rows as the early-end run: the same first decisions
    assert eq(a["batch"].a_d[:N67], R["early"]["batch"].a_d)


# ------------------------------------------------------------------ 4. equivalences with the early-end path
@pytest.mark.parametrize("case", ROLL, ids=lambda c: c[0])
def test_one_lane_is_early_end(case):
    R = runs(case)
    a, e = R["one"], R["early"]
    assert e["batch"].len.tolist() == R["lens"].tolist()
    buckets_equal(a["buckets"], e["buckets"])
    assert bool(a["buckets"][2]["rew_sums"][:2].abs().sum() > 0)


def test_one_lane_lengths_are_the_effective_ones():
    """early_end leaves a running stream's len 0; the closed lane carries its effective length and cut"""
    R = runs(ROLL[0])
    b, T = R["one"]["batch"], ROLL[0][5]
    assert b.len.tolist() == np.where(R["lens"] > 0, R["lens"], T).tolist() and b.cut.tolist() == (R["lens"] == 0).astype(int).tolist()


@pytest.mark.parametrize("case", ROLL, ids=lambda c: c[0])
def test_never_done_is_early_end(case):
    from mhppo.external import ExternalRollout
    from mhppo.rollout import bucket_segments
    from test_bootstrap_gpu import TruncSim
    R = runs(case)
    T = case[5]
    buckets_equal(R["never3"]["buckets"], R["never_early"]["buckets"])
    b = R["never3"]["batch"]
    assert b.len.reshape(3, N67).tolist() == [[T] * N67, [0] * N67, [0] * N67] and b.cut[:N67].tolist() == [1] * N67
    # bootstrapped: the cut at T is a truncation, its targets start from V of finish()'s rows
    got = {}
    for name, kw in (("lanes", dict(auto_reset=4)), ("early", dict(early_end=True))):
        ext = ExternalRollout(R["pol"], N67, T=T, seed=SEED, bootstrap=True, **kw)
        sim = TruncSim(make_env(case, N67), R["never"], np.zeros_like(R["never"]))
        bb = ext.collect(sim, ITER)
        assert bb.feat_tail is not None
        got[name] = bucket_segments(bb, status=ext.status, boot=critics())
    buckets_equal(got["lanes"], got["early"])
    assert not eq(got["lanes"][0]["ret"], R["never3"]["buckets"][0]["ret"])


# ------------------------------------------------------------------ 5. the restart decision
def test_restart_decision_is_sample_decide_at_the_counter():
    from mhppo import _lib
    from mhppo.external import ExternalRollout
    from mhppo.policy import noise_key
    case = ROLL[1]
    R = runs(case)
    T, E, first_env = 8, 3, 5
    pol = R["pol"]
    S, P = pol.n_slots, pol.nb_ped
    ext = ExternalRollout(pol, N67, T=T, seed=SEED, first_env=first_env, auto_reset=E)
    done = R["done"]
    want = lane_lists(done, E, T)
    sim = ScheduledSim(make_env(case, N67), done)
    obs = sim.reset()
    ext.begin(obs, ITER)
    key = noise_key(SEED, ITER)
    n_restart = n_keep = 0
    for t in range(T):
        prev = {k: getattr(ext.session.decision, k).clone() for k in DEC}
        actions = ext.act(obs, t)
        if t >= 1:
            u = torch.empty((N67, S, P), dtype=torch.float32, device="cuda")
            off = ((t + 1) << 40) + (1 << 39) + first_env * S * P
            _lib.check(_lib.lib().mhppo_philox_uniform(key, off, _lib.ptr(u), u.numel(), _lib.stream_ptr()))
            fresh = pol.sample_decide(obs, u=u, want_probs=True, want_features=True)
            for r in range(N67):
                e = [i for i, x in enumerate(want[r]) if x[0] == t and i > 0]
                src = fresh if e else types.SimpleNamespace(**prev)
                for k in DEC:
                    assert eq(getattr(ext.session.decision, k)[r], getattr(src, k)[r]), (t, r, k)
                    if e:
                        assert eq(ext.lanes[k][e[0] * N67 + r], getattr(fresh, k)[r]), (t, r, k)
                n_restart += bool(e)
                n_keep += not e
        obs, rew, rl, d = sim.step(actions)
        ext.record(rew, rl, d)
    assert n_restart > 10 and n_keep > 10
    assert ext.batch().t0.reshape(E, N67)[1:].max() > 1


def test_restart_tape_is_read_for_restarting_streams_only():
    from mhppo.external import ExternalRollout
    case = ROLL[0]
    R = runs(case)
    pol, T = R["pol"], 4
    S, P = pol.n_slots, pol.nb_ped
    done = np.zeros((T, N67), dtype=bool)
    done[0, ::2] = True  # the even streams restart at step 1
    ext = ExternalRollout(pol, N67, T=T, seed=SEED, auto_reset=2)
    sim = ScheduledSim(make_env(case, N67), done)
    obs = sim.reset()
    d0 = ext.begin(obs, ITER)
    first = d0.a_d.clone()
    obs, rew, rl, d = sim.step(ext.act(obs, 0))
    ext.record(rew, rl, d)
    forced = 1 - first  # every decision flipped
    ext.act(obs, 1, forced=forced)
    now = ext.session.decision.a_d
    assert eq(now[::2], forced[::2]) and eq(now[1::2], first[1::2])
    assert eq(ext.lanes["a_d"][N67:][::2], forced[::2]) and not bool(ext.lanes["a_d"][N67:][1::2].any())
    assert eq(ext.lanes["a_d"][:N67], first)


# ------------------------------------------------------------------ 6. training
def test_train_external_auto_reset_equals_by_hand():
    from mhppo.algo import Algo_PPO
    from mhppo.external import ExternalRollout
    from mhppo.models import Model_PPO
    from mhppo.rollout import bucket_segments_lanes_torch
    case = ("scalable", 4, 3, 2, 0, 20)
    T, E = case[5], 2
    lens, done = schedule(N67, T)
    torch.manual_seed(3)
    a = Algo_PPO(Model_PPO, make_env(case, N67), seed=6, verbose=False, save_curves=False)
    b = Algo_PPO(Model_PPO, make_env(case, N67), seed=6, verbose=False, save_curves=False)
    for na, nb in zip(a.nets(), b.nets()):
        nb.load_state_dict(na.state_dict())
    before = {k: v.clone() for k, v in algo_state(a).items()}
    sim_a, sim_b = ScheduledSim(make_env(case, N67), done), ScheduledSim(make_env(case, N67), done)
    a.train_external(sim_a, 2, M=N67, auto_reset=E)
    assert a._external[0] == (N67, T, True, ("auto_reset", E)) and a.rollout.batch.lanes == E
    n_seg = a.rollout.cross["n_seg"] + a.rollout.wait["n_seg"]
    assert a.rollout.cross["rows"] + a.rollout.wait["rows"] < n_seg * T
    assert int(a.rollout.batch.exist[N67:].sum()) > 0  # second episodes were played
    r = b.rollout
    r.fix_bucket, r.gae = b.fix_bucket, None
    ext = ExternalRollout(b.policy(), N67, T=T, auto_reset=E)
    ext.session.first_env = int(b.venv.cfg.env_id_offset)
    for ep in range(2):
        ext.session.seed = int(r.seed)
        r.batch = ext.collect(sim_b, r.iteration)
        r.iteration += 1
        r.cross, r.wait, r.choice = bucket_segments_lanes_torch(r.batch, fix_bucket=r.fix_bucket, status=ext.status)
        b._after_collect(ep, reset_env=False)
    b._finish_train()
    sa, sb = algo_state(a), algo_state(b)
    assert set(sa) == set(sb)
    for k in sa:
        assert eq(sa[k], sb[k]), k
    assert any(not eq(sa[k], before[k]) for k in before if k.startswith("net"))
    ca, cb = a.curves(), b.curves()
    print("curves", ca, cb)
    assert ca == cb and len(ca[2]) == 2
    # values that hash like the cached key's E are refused, not served from the cache
    for bad in (float(E), True, 0, "2"):
        with pytest.raises(ValueError):
            a.train_external(sim_a, 1, M=N67, auto_reset=bad)
    assert a._external[0] == (N67, T, True, ("auto_reset", E)) and a.total_loop == 2
    # auto_reset is part of the cache key
    a.train_external(ScheduledSim(make_env(case, N67), done), 1, M=N67, early_end=True)
    assert a._external[0] == (N67, T, True) and getattr(a.rollout.batch, "lanes", None) is None
    with pytest.raises(ValueError):
        a.train_external(sim_a, 1, M=N67, auto_reset=E, early_end=False)
    g = Algo_PPO(Model_PPO, make_env(case, N67), seed=6, verbose=False, save_curves=False, gae_lambda=0.95)
    with pytest.raises(ValueError):
        g.train_external(sim_a, 1, M=N67, auto_reset=E)


# ------------------------------------------------------------------ 7. misuse
def test_api_rejects_misuse():
    from mhppo.env import VecCrosswalk
    from mhppo.external import ExternalRollout
    from mhppo.policy import Policy
    from mhppo.rollout import bucket_segments
    from test_policy_gpu import nets
    ac, aw, ad = nets(17)
    pol = Policy("coop", 2, 1, 2, ac, aw, ad)
    M, S, T = 5, pol.n_slots, 3
    obs = VecCrosswalk("coop", M, 2, 1, 2, seed_base=3).reset()
    rew = torch.zeros((M, S), dtype=torch.float64, device="cuda")
    done = torch.zeros(M, dtype=torch.bool, device="cuda")
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            ExternalRollout(pol, M, T=T, auto_reset=bad)
    with pytest.raises(ValueError):
        ExternalRollout(pol, M, T=T, auto_reset=2, compact=True)
    with pytest.raises(ValueError):  # the counter bound: (first_env + M) S P >= 2^39
        ExternalRollout(pol, M, T=T, auto_reset=2, first_env=2**39 // (S * pol.nb_ped))
    ext = ExternalRollout(pol, M, T=T, auto_reset=2, bootstrap=True)
    assert ext.early_end and ext.compact is False and ext.len is None
    with pytest.raises(ValueError):
        ext.act(obs, 0)  # before begin
    ext.begin(obs, 0)
    with pytest.raises(ValueError):
        ext.batch()  # no step recorded
    with pytest.raises(ValueError):
        ext.act(obs, 1)  # steps are acted on in order
    ext.act(obs, 0)
    with pytest.raises(ValueError):
        ext.act(obs, 0)  # and once each
    with pytest.raises(ValueError):
        ext.record(rew, rew, done, done)  # a truncated flag
    with pytest.raises(ValueError):
        ext.record(rew, rew)  # done is required
    ext.record(rew, rew, done)
    with pytest.raises(ValueError):
        ext.record(rew, rew, done)  # recorded already
    ext.session.first_env = 2**39  # set later, as train_external does: caught at the restart draw
    with pytest.raises(ValueError):
        ext.act(obs, 1)
    ext.session.first_env = 0
    ext.act(obs, 1)
    with pytest.raises(ValueError):
        ext.batch()  # step 1 acted on and not recorded
    ext.record(rew, rew, ~done)
    b = ext.batch()
    assert b.steps == 2 and b.len.tolist() == [2] * M + [0] * M and b.cut.tolist() == [0] * (2 * M)
    with pytest.raises(ValueError):
        bucket_segments(b, gae=(None, None, GAMMA, 0.95))  # gae_lambda with auto_reset
    fixed = ExternalRollout(pol, M, T=T, early_end=True)
    fixed.begin(obs, 0)
    with pytest.raises(ValueError):
        fixed.act(obs, 0, forced=torch.zeros((M, S, pol.nb_ped), dtype=torch.int32, device="cuda"))  # auto_reset only
    with pytest.raises(ValueError):
        ext.collect(None, 0, check_every=0)


def test_check_every_stops_once_every_stream_idles():
    from mhppo.external import ExternalRollout
    case = ROLL[0]
    R = runs(case)
    T, E = case[5], 2
    done = np.zeros((T, N67), dtype=bool)
    done[2], done[4 + np.arange(N67) % 3, np.arange(N67)] = True, True  # the second episodes end at steps 4 .. 6
    ext = ExternalRollout(R["pol"], N67, T=T, seed=SEED, auto_reset=E)
    sim = ScheduledSim(make_env(case, N67), done)
    b = ext.collect(sim, ITER, check_every=4)
    assert b.steps == 8 == sim.t and not bool(b.cut.any())  # the first check at or after step 7
    sim = ScheduledSim(make_env(case, N67), done)
    assert ext.collect(sim, ITER).steps == T == sim.t  # no host read: T steps


def test_abi_rejects_bad_input():
    from mhppo import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    M, S, T, E = 4, 2, 3, 2
    NS, NL = M * S, E * M * S
    f = lambda n: torch.full((n,), SENT, dtype=torch.float32, device="cuda")
    d = lambda n: torch.full((n,), SENT, dtype=torch.float64, device="cuda")
    i32 = lambda n: torch.full((n,), int(SENT), dtype=torch.int32, device="cuda")
    i64 = lambda n: torch.full((n,), int(SENT), dtype=torch.int64, device="cuda")
    u8 = lambda n: torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    dec = lambda n: types.SimpleNamespace(a_d=i32(n * S * P2), logp_d=f(n * S * P2), probs=f(n * S * P2 * 2),
                                          feat_d=f(n * S * P2 * DC), closest=i32(n * S), exist=u8(n * S))
    lanes_d, first, now = dec(E * M), dec(M), dec(M)
    lanes = dict(lanes_d.__dict__, ep_min=d(NL), t0=i32(E * M), len=i32(E * M), cur=i32(2 * M))
    ls, fs, ns = lanes_struct(lanes), dec_struct(first), dec_struct(now)
    hole = lanes_struct(lanes)
    hole.t0 = None
    fhole = dec_struct(first)
    fhole.probs = None
    B, R = ctypes.byref, []
    begin = lambda ls=ls, E=E, M=M, S=S, P=P2, dc=DC, fs=fs: L.mhppo_lanes_begin(B(ls), E, M, S, P, dc, B(fs), st)
    R += [begin(E=0), begin(M=-1), begin(S=0), begin(M=2**30, S=2), begin(E=2**16, M=2**15), begin(P=0), begin(dc=0),
          begin(ls=hole), begin(fs=fhole), L.mhppo_lanes_begin(None, E, M, S, P2, DC, B(fs), st)]
    restart = lambda ls=ls, E=E, M=M, S=S, t=1, T=T, fs=fs, ns=ns: L.mhppo_lanes_restart(B(ls), E, M, S, P2, DC, t, T, B(fs),
                                                                                       B(ns), st)
    R += [restart(E=0), restart(M=-1), restart(S=0), restart(t=0), restart(t=T), restart(ls=hole), restart(fs=fhole),
          restart(ns=fhole)]
    src = dict(act=f(NS), logp=f(NS), feat_c=f(NS * 13), rew=d(NS), rew_light=d(NS))
    dst = dict(obs=f(T * NS * 13), act=f(T * NS), logp=f(T * NS), rew=d(T * NS))
    done = torch.ones(M, dtype=torch.uint8, device="cuda")

    def record(ls=ls, E=E, M=M, S=S, t=0, T=T, done=done, **null):
        a = {**src, **{"d_" + k: v for k, v in dst.items()}}
        a = {k: (None if k in null else p(v)) for k, v in a.items()}
        return L.mhppo_lanes_record(B(ls), E, M, S, t, T, a["act"], a["logp"], a["feat_c"], a["rew"], a["rew_light"],
                                    a["d_obs"], a["d_act"], a["d_logp"], a["d_rew"], p(done), st)

    R += [record(E=0), record(M=-1), record(S=0), record(M=2**30, S=2), record(t=-1), record(t=T), record(done=None),
          record(ls=hole)]
    R += [record(**{k: 1}) for k in list(src) + ["d_" + k for k in dst]]
    ln, cut = i32(E * M), u8(E * M)
    close = lambda ls=ls, E=E, M=M, k=1, ln=ln, cut=cut: L.mhppo_lanes_close(B(ls), E, M, k, T, p(ln), p(cut), st)
    R += [close(E=0), close(M=-1), close(k=0), close(k=T + 1), close(ln=None), close(cut=None), close(ls=hole)]
    assert b"lanes_close" in L.mhppo_last_error()
    pos, ret = i64(NL), f(T * NS)
    scan = lambda rew=dst["rew"], ret=ret, M=M, S=S, E=E, T=T, pos=pos, t0=lanes["t0"], ln=ln, cut=cut: \
        L.mhppo_returns_scan_tm_lanes(p(rew), p(ret), M, S, E, T, GAMMA, p(pos), p(t0), p(ln), p(cut), None, st)
    R += [scan(E=0), scan(M=-1), scan(S=0), scan(T=0), scan(M=2**30, S=2), scan(rew=None), scan(ret=None), scan(pos=None),
          scan(t0=None), scan(ln=None), scan(cut=None)]
    one = _lib.BucketDst(*[dst[k].data_ptr() for k in ("obs", "act", "logp", "act", "rew")])
    two = (_lib.BucketDst * 2)(one, one)
    sums, work, bucket = d(2), d(16), torch.zeros(NL, dtype=torch.int8, device="cuda")
    a = dict(row0=pos, bucket=bucket, t0=lanes["t0"], ln=ln, obs=dst["obs"], act=dst["act"], logp=dst["logp"], ret=ret,
             rew=dst["rew"])

    def scatter(M=M, S=S, E=E, T=T, dst_=two, sums=sums, work=work, **null):
        q = {k: (None if k in null else p(v)) for k, v in a.items()}
        return L.mhppo_bucket_scatter_lanes(q["row0"], q["bucket"], q["t0"], q["ln"], M, S, E, T, q["obs"], q["act"], q["logp"],
                                            q["ret"], q["rew"], dst_, p(sums), p(work), st)

    R += [scatter(E=0), scatter(M=-1), scatter(S=0), scatter(T=0), scatter(dst_=None), scatter(sums=None), scatter(work=None)]
    R += [scatter(**{k: 1}) for k in a]
    assert all(rc == -1 for rc in R), R
    assert b"bucket_scatter_lanes" in L.mhppo_last_error()
    # M == 0 launches nothing, whatever the pointers
    assert begin(M=0) == 0 and restart(M=0) == 0 and record(M=0) == 0 and close(M=0) == 0 and scan(M=0) == 0 and scatter(M=0) == 0
    assert L.mhppo_lanes_begin(None, E, 0, S, P2, DC, None, st) == 0
    torch.cuda.synchronize()
    every = list(lanes.values()) + list(first.__dict__.values()) + list(now.__dict__.values()) + list(dst.values())
    for v in every + [ln, cut, pos, ret, sums, work]:
        want = SENT if v.dtype.is_floating_point else (77 if v.dtype == torch.uint8 else int(SENT))
        assert bool((v == want).all())
