"""Truncation bootstrap on the GPU (mhppo_boot_values, mhppo_returns_scan_tm_boot, mhppo_gae_tm_boot;
ExternalRollout(early_end=True, bootstrap=True), Algo_PPO.train_external(bootstrap=True)).  Every comparison is
bit for bit.  done comes from the early-end tests' host-known schedule, truncated from a second one:
  1. mhppo_boot_values against boot_values_torch and against forward_rows on the rows a restatement of the
     rule selects, between sentinels, every row the rule must not select NaN;
  2. both scans with v_boot against their torch specifications; v_boot NULL = the _len entry points;
  3. ExternalRollout(bootstrap=True) on a VecCrosswalk: native = specification; nothing truncated = early_end
     alone; every truncated segment's targets start from V of its successor row in a never-done twin run (the
     test that needs the feature: the parent has no such argument); batch() at k < T with and without finish;
     collect() with check_every;
  4. train_external(bootstrap=True) against the same iterations made by hand on the torch bucketing;
  5. misuse of the Python API and of the ABI."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from test_early_end_gpu import (GAMMA, ITER, N, ROLL, SEED, SENT, ScheduledSim, buckets_equal, critics, cu, eq,
                                plan_inputs, runs, scan_lengths, schedule)
from test_external_gpu import BATCH_KEYS, TM_KEYS, algo_state, make_env
from test_policy_gpu import guarded, guards_intact, same_bits

pytestmark = pytest.mark.gpu
T5 = 5


# ------------------------------------------------------------------ 1. mhppo_boot_values vs spec
def boot_inputs(M, S, k, compact, kind, cut, tail, trunc_on=True):
    """The kernel's operands for the early-end schedule (stream r ends at 1 + 7 r mod T, every fifth never;
    trunc[r] = r & 1), with finite rows exactly where a restatement of the rule selects one and NaN in every
    other record row and tail row.  Returns the operands, the selection and the expected values' rows."""
    NS = M * S
    lens, _ = schedule(M, T5)
    r_ = np.arange(M)
    trunc = ((r_ & 1) if trunc_on else np.zeros(M)).astype(np.uint8)
    pos, bucket, rec_of = plan_inputs(M, S, compact, "none" if kind == "unused" else kind, 2)
    s = torch.arange(NS)
    r = s // S
    col = s if rec_of is None else rec_of.cpu().long()
    has = col >= 0
    colc = col.clamp_min(0)
    ln = torch.from_numpy(lens)[r]
    ended = (ln >= 1) & (ln <= k)
    L = torch.where(ended, ln, torch.full_like(ln, k))
    tr = torch.where(ended, torch.from_numpy(trunc)[r] != 0, torch.full_like(ended, bool(cut)))
    sel = has & (pos.cpu()[colc] >= 0) & tr & ((L < k) | bool(tail))
    g = torch.Generator().manual_seed(1000 * M + 10 * k + S)
    obs = torch.full((T5, NS, 13), float("nan"))
    feat_tail = torch.full((NS, 13), float("nan"))
    rows = torch.zeros((NS, 13))
    rows[sel] = torch.randn((int(sel.sum()), 13), generator=g)
    rec = sel & (L < k)
    obs[L[rec], colc[rec]] = rows[rec]
    feat_tail[sel & ~rec] = rows[sel & ~rec]
    ops = dict(pos=pos, bucket=bucket, rec_of=rec_of, len=cu(lens, torch.int32), trunc=cu(trunc), obs=obs.cuda(),
               tail=feat_tail.cuda() if tail else None)
    return ops, dict(sel=sel, col=col, has=has, wait=bucket.cpu()[colc] != 0, rows=rows, L=L)


def run_boot(M, S, k, ops, cut):
    from mhppo import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    c0, c1 = critics()
    d0, k0 = c0.mlp_desc()
    d1, k1 = c1.mlp_desc()
    buf, v = guarded(M * S, torch.float32, SENT)
    assert L.mhppo_boot_values(ctypes.byref(d0), ctypes.byref(d1), p(ops["pos"]), p(ops["bucket"]), p(ops["rec_of"]),
                               p(ops["len"]), p(ops["trunc"]), M, S, k, cut, p(ops["obs"]), p(ops["tail"]), p(v), st) == 0
    torch.cuda.synchronize()
    assert guards_intact(buf, M * S, SENT)
    return v


def check_boot_values(M, S, k, compact, kind, cut, tail, trunc_on=True):
    from mhppo.rollout import boot_values, boot_values_torch
    c0, c1 = critics()
    ops, x = boot_inputs(M, S, k, compact, kind, cut, tail, trunc_on)
    NS = M * S
    spec = boot_values_torch(c0, c1, ops["pos"], ops["bucket"], ops["rec_of"], ops["len"], ops["trunc"], M, S, k, cut,
                             ops["obs"], ops["tail"])
    assert bool(torch.isfinite(spec).all())  # a wrong gather in the specification itself would be a NaN
    # the restated rule: V of the selected rows by forward_rows, everything else 0
    V = [c.forward_rows(x["rows"].cuda()).cpu() for c in (c0, c1)]
    want = torch.zeros(NS + 1)
    want[torch.where(x["has"], x["col"], NS)] = torch.where(x["sel"], torch.where(x["wait"], V[1], V[0]), torch.zeros(()))
    assert eq(spec, want[:NS])
    got = run_boot(M, S, k, ops, cut)
    n_rec = int(x["has"].sum())  # columns [n_rec, NS) hold no record: not touched
    assert eq(got[:n_rec], spec[:n_rec]) and bool((got[n_rec:] == SENT).all()), (kind, cut, tail)
    assert eq(boot_values(c0, c1, ops["pos"], ops["bucket"], ops["rec_of"], ops["len"], ops["trunc"], M, S, k, cut,
                          ops["obs"], ops["tail"]), spec)
    return x, spec


@pytest.mark.parametrize("kind", ["mixed", "all_cross", "all_wait", "unused"])
@pytest.mark.parametrize("compact", [False, True], ids=["identity", "compact"])
@pytest.mark.parametrize("k", [1, 5, 3])
@pytest.mark.parametrize("M,S", [(1, 1), (11, 3), (85, 3), (1031, 8)])
def test_boot_values_equals_spec(M, S, k, compact, kind):
    """(11, 3): stream 10's segments 30..32 straddle a 32-segment tile.  (85, 3): the record kernel's two-block
    case, 8 tiles in two blocks here.  (1031, 8): 258 tiles in 65 blocks, below the cap of 512 blocks: one tile
    per wave; the capped regime is test_boot_values_past_the_grid_cap."""
    if (M, S) == (11, 3):
        assert 10 * S <= 31 < 32 <= 10 * S + S - 1
    seen = dict(wait=0, cross=0, rec=0, tail=0)  # selected segments over the four combinations
    for cut in (0, 1):
        for tail in (False, True):
            x, spec = check_boot_values(M, S, k, compact, kind, cut, tail)
            sel, L = x["sel"], x["L"]
            seen["wait"] += int((sel & x["wait"]).sum())
            seen["cross"] += int((sel & ~x["wait"]).sum())
            seen["rec"] += int((sel & (L < k)).sum())
            seen["tail"] += int((sel & (L == k)).sum())
            assert tail or not bool((sel & (L == k)).any())  # without a tail no segment of length k is selected
            if kind == "unused":
                assert not bool(spec.any())
    if kind == "unused":
        assert not any(seen.values())
    elif M >= 85:  # both critics, record rows (k = 1 has none: no L < k) and tail rows
        assert (seen["wait"] > 0) == (kind != "all_cross") and (seen["cross"] > 0) == (kind != "all_wait"), seen
        assert (seen["rec"] > 0) == (k > 1) and seen["tail"] > 0, seen


@pytest.mark.parametrize("compact", [False, True], ids=["identity", "compact"])
def test_nothing_truncated_writes_zeros(compact):
    """no truncated flag and a terminal cut: zeros in every column that holds a record, the rest untouched,
    whatever the rows hold (all NaN here)"""
    x, spec = check_boot_values(85, 3, 3, compact, "mixed", 0, True, trunc_on=False)
    assert not bool(x["sel"].any()) and not bool(spec.any())


def test_boot_values_past_the_grid_cap():
    """8200 x 8 segments are 2050 tiles, 513 blocks' worth: the grid is capped at 512 and block 0's waves walk a
    second tile each"""
    M, S = 8200, 8
    assert (M * S + 31) // 32 > 4 * 512
    x, spec = check_boot_values(M, S, 3, True, "mixed", 1, True)
    last = x["sel"] & (torch.arange(M * S) >= 2048 * 32)
    assert bool(last.any()) and bool(spec.cpu()[x["col"][last]].ne(0).all())


# ------------------------------------------------------------------ 2. the two scans
@pytest.mark.parametrize("T", (1, 7, 19))
@pytest.mark.parametrize("B", (1, 33, 100))
def test_scans_with_v_boot_equal_spec(B, T):
    from mhppo import _lib
    from mhppo.rollout import gae_targets_tm, gae_targets_torch, returns_scan_tm
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    g = torch.Generator().manual_seed(B * 100 + T + 7)
    rew_h = torch.randn((T, B), generator=g, dtype=torch.float64)
    X = torch.randn((T, B, 13), generator=g).cuda()
    vb_h = torch.randn(B, generator=g) * 3.0
    ln_h, used_h = scan_lengths(B, T, B + T)
    if B >= 33:
        assert bool((vb_h > 0).any()) and bool((vb_h < 0).any())
    if B >= 100:  # a column of no steps with a non-zero v_boot
        assert (ln_h == 0).any() and bool((vb_h[torch.from_numpy(ln_h == 0)] != 0).all())
    ln, rew, vb = cu(ln_h), rew_h.cuda(), vb_h.cuda()
    dead = torch.arange(T)[:, None] >= torch.from_numpy(ln_h.astype(np.int64))[None, :]
    rew_nan = rew_h.clone()
    rew_nan[dead] = float("nan")  # nothing at or past a length is read into a result
    # the reward-to-go: the CPU form of returns_scan_tm is the float64 specification
    got = returns_scan_tm(rew_nan.cuda(), GAMMA, len_rec=ln, v_boot=vb)
    assert eq(got, returns_scan_tm(rew_h, GAMMA, len_rec=torch.from_numpy(ln_h), v_boot=vb_h))
    assert not bool(got.cpu()[dead].any())
    if (ln_h > 0).any():
        assert not eq(got, returns_scan_tm(rew, GAMMA, len_rec=ln))
    assert eq(returns_scan_tm(rew, GAMMA, v_boot=vb), returns_scan_tm(rew_h, GAMMA, v_boot=vb_h))  # len_rec NULL: T steps
    out = torch.full((T, B), SENT, dtype=torch.float32, device="cuda")
    assert L.mhppo_returns_scan_tm_boot(p(rew), p(out), B, T, GAMMA, p(ln), None, st) == 0  # v_boot NULL
    assert eq(out, returns_scan_tm(rew, GAMMA, len_rec=ln))
    # GAE: V from the kernel's own value_tm; the recurrence from gae_targets_torch
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
                                  len_rec=ln_u, v_boot=vb)
        assert eq(val, torch.where(live, val_full, torch.zeros_like(val_full))), with_pos
        len_used = torch.where(used, ln_u, torch.zeros_like(ln_u))
        want = gae_targets_torch(rew, val_full, GAMMA, 0.95, len_rec=len_used, v_boot=vb)
        assert eq(ret, want), with_pos
        assert not bool(ret[~live].any()) and bool(ret[live].any())
        assert not eq(ret, gae_targets_torch(rew, val_full, GAMMA, 0.95, len_rec=len_used))
        # v_boot NULL: mhppo_gae_tm_len's bits
        r2 = torch.full((T, B), SENT, dtype=torch.float32, device="cuda")
        v2 = torch.full((T, B), SENT, dtype=torch.float32, device="cuda")
        d0, k0 = c0.mlp_desc()
        d1, k1 = c1.mlp_desc()
        assert L.mhppo_gae_tm_boot(ctypes.byref(d0), ctypes.byref(d1) if with_pos else None, p(X), p(rew), p(pos), p(bucket),
                                   B, T, GAMMA, 0.95, p(r2), p(v2), p(ln_u), None, st) == 0
        r3, v3 = gae_targets_tm(X, rew, c0, c1 if with_pos else None, pos, bucket, GAMMA, 0.95, want_value=True,
                                len_rec=ln_u)
        assert eq(r2, r3) and eq(v2, v3)


# ------------------------------------------------------------------ 3. ExternalRollout(bootstrap=True)
def trunc_schedule(lens, T, zero=False):
    """truncated bool [T, M]: r & 1 at the step of stream r's first done and the opposite at every other step,
    so only a reading at that step gives trunc[r] = r & 1; streams that never end raise it without a done"""
    M = lens.shape[0]
    want = (np.arange(M) & 1).astype(bool)
    at_end = np.arange(T)[:, None] == lens[None, :] - 1
    tr = np.where(at_end, want[None, :], ~want[None, :])
    return np.zeros_like(tr) if zero else tr


class TruncSim(ScheduledSim):
    """ScheduledSim whose step also returns the schedule's truncated, the Gymnasium-style fifth value"""

    def __init__(self, env, done, trunc):
        super().__init__(env, done)
        self.trunc = torch.from_numpy(trunc).cuda()
        self.last_obs = None

    def step(self, actions):
        t = self.t
        obs, rew, rl, done = super().step(actions)
        self.last_obs = obs.clone()
        return obs, rew, rl, done, self.trunc[t].clone()


@functools.lru_cache(maxsize=None)
def boot_runs(case):
    """Once per case: the bootstrapped run on the native pass and on its specification, and the run in which
    nothing is truncated.  The early-end tests' runs(case) gives the policy, the schedule, the early_end-only run
    ("sched") and the never-done twin ("never")."""
    from mhppo.external import ExternalRollout
    from mhppo.rollout import bucket_segments, bucket_segments_ragged_torch
    R = runs(case)
    T = case[5]
    out = dict(R=R, trunc=trunc_schedule(R["lens"], T))

    def run(name, native, cut, tr, bucketing):
        ext = ExternalRollout(R["pol"], N, T=T, seed=SEED, native=native, early_end=True, bootstrap=True, cut_truncates=cut)
        sim = TruncSim(make_env(case), R["done"], tr)
        b = ext.collect(sim, ITER)
        out[name] = dict(ext=ext, sim=sim, batch=b, buckets=bucketing(b, status=ext.status, boot=critics()))

    run("boot", True, True, out["trunc"], bucket_segments)
    run("spec", False, True, out["trunc"], bucket_segments_ragged_torch)
    run("zero", True, False, trunc_schedule(R["lens"], T, zero=True), bucket_segments)
    return out


def want_trunc(lens):
    return np.where(lens > 0, np.arange(lens.shape[0]) & 1, 0)


@pytest.mark.parametrize("case", ROLL, ids=lambda c: c[0])
def test_native_equals_spec_on_an_env(case):
    B = boot_runs(case)
    a, b = B["boot"], B["spec"]
    assert a["batch"].cut_truncates is True and a["batch"].steps == case[5]
    for k in BATCH_KEYS + TM_KEYS + ("len", "trunc", "feat_tail"):
        assert eq(getattr(a["batch"], k), getattr(b["batch"], k)), k
    lens = B["R"]["lens"]
    assert a["batch"].len.tolist() == lens.tolist() and a["batch"].trunc.tolist() == want_trunc(lens).tolist()
    assert a["batch"].trunc.dtype == torch.uint8 and tuple(a["batch"].feat_tail.shape) == (N, a["batch"].S, 13)
    buckets_equal(a["buckets"], b["buckets"])


@pytest.mark.parametrize("case", ROLL, ids=lambda c: c[0])
def test_nothing_truncated_is_early_end_alone(case):
    from mhppo.rollout import bucket_segments
    B = boot_runs(case)
    z, e = B["zero"], B["R"]["sched"]
    assert not bool(z["batch"].trunc.any()) and z["batch"].cut_truncates is False
    buckets_equal(z["buckets"], e["buckets"])
    c0, c1 = critics()
    gae = (c0, c1, GAMMA, 0.95)
    buckets_equal(bucket_segments(z["batch"], gae=gae, boot=(c0, c1)), bucket_segments(e["batch"], gae=gae))


def check_bootstrap(B, case, got, base, lens_eff, k, tr_stream, tail_rows):
    """Every segment's ret in `got` by a float64 loop started from V of its successor row where the stream was
    truncated -- record L of the never-done twin for L < k, tail_rows [NS, 13] (None: no bootstrap) for L == k --
    and from 0 where it ended; every other key of `got` as in `base`, the same batch bucketed without boot.
    Returns the number of bootstrapped segments per bucket."""
    from mhppo.rollout import bucket_segments_torch
    R = B["R"]
    T = case[5]
    nb = R["never"]["batch"]
    S, NS = nb.S, N * nb.S
    plan = {}
    bucket_segments_torch(nb, plan_out=plan)
    exist = nb.exist.reshape(-1).bool().cpu()
    wait = plan["wait"].cpu()
    col = torch.arange(NS) if nb.rec_of is None else nb.rec_of.long().cpu()
    seg_len, seg_tr = np.repeat(lens_eff, S), np.repeat(tr_stream, S)
    twin = nb.obs_c_tm.reshape(T, NS, 13).cpu()
    rows, have = torch.zeros((NS, 13)), np.zeros(NS, dtype=bool)
    for s in np.nonzero(exist.numpy() & seg_tr)[0]:
        if seg_len[s] < k:
            rows[s], have[s] = twin[seg_len[s], col[s]], True
        elif tail_rows is not None:
            rows[s], have[s] = tail_rows[s], True
    V = [c.forward_rows(rows.cuda()).cpu().numpy() for c in critics()]
    counts = []
    for i, mask in enumerate((exist & ~wait, exist & wait)):
        full, g = R["never"]["buckets"][i], got[i]
        rew = full["rew"].cpu().reshape(full["n_seg"], T).numpy()
        ret = g["ret"].cpu().numpy()
        want, row = [], 0
        for j, s in enumerate(np.nonzero(mask.numpy())[0]):
            Lj = int(seg_len[s])
            G, r = (float(np.float64(V[i][s])) if have[s] else 0.0), np.zeros(Lj, dtype=np.float32)
            if have[s]:  # the bucket's last row of the segment, exactly
                assert ret[row + Lj - 1] == np.float32(rew[j, Lj - 1] + GAMMA * np.float64(V[i][s])), (i, s)
            for t in range(Lj - 1, -1, -1):
                G = rew[j, t] + GAMMA * G
                r[t] = np.float32(G)
            want.append(r)
            row += Lj
        assert same_bits(ret, np.concatenate(want)), i
        for key in ("obs", "act", "logp", "rew"):
            assert eq(g[key], base[i][key]), (i, key)
        assert g["rows"] == base[i]["rows"] and g["n_seg"] == base[i]["n_seg"]
        counts.append((int(have[mask.numpy()].sum()), int((~have)[mask.numpy()].sum())))
    for key in base[2]:
        assert got[2][key] == base[2][key] if key == "n_seg" else eq(got[2][key], base[2][key]), key
    return counts


@pytest.mark.parametrize("case", ROLL, ids=lambda c: c[0])
def test_truncated_segments_bootstrap_from_the_successor(case):
    B = boot_runs(case)
    R, a = B["R"], B["boot"]
    T, lens = case[5], R["lens"]
    lens_eff = np.where(lens > 0, lens, T)
    tr_stream = np.where(lens > 0, (np.arange(N) & 1) == 1, True)  # a stream cut at T is truncated
    # the tail rows do not depend on the noise: sample_act on the last rows with another tape
    d = a["ext"].session.decision
    other = R["pol"].sample_act(a["sim"].last_obs, d.a_d, d.closest,
                                eps=torch.ones((N, a["batch"].S), dtype=torch.float32, device="cuda"))
    assert eq(other.feat_c.reshape(N, -1, 13), a["batch"].feat_tail)
    counts = check_bootstrap(B, case, a["buckets"], R["sched"]["buckets"], lens_eff, T, tr_stream,
                             a["batch"].feat_tail.reshape(-1, 13).cpu())
    assert all(nb > 0 and nt > 0 for nb, nt in counts), counts  # bootstrapped and terminal segments in both buckets
    assert ((lens_eff == T) & tr_stream).any() and ((lens_eff < T) & tr_stream).any()
    for i in range(2):
        assert not eq(a["buckets"][i]["ret"], R["sched"]["buckets"][i]["ret"])


@pytest.mark.parametrize("finish", [True, False], ids=["finish", "no_finish"])
@pytest.mark.parametrize("case", ROLL, ids=lambda c: c[0])
def test_batch_before_T(case, finish):
    from mhppo.external import ExternalRollout
    from mhppo.rollout import bucket_segments
    B = boot_runs(case)
    R = B["R"]
    T, k, lens = case[5], 7, R["lens"]
    ext = ExternalRollout(R["pol"], N, T=T, seed=SEED, early_end=True, bootstrap=True)
    sim = TruncSim(make_env(case), R["done"], B["trunc"])
    obs = sim.reset()
    ext.begin(obs, ITER)
    for t in range(k):
        obs, rew, rl, d, tr = sim.step(ext.act(obs, t))
        ext.record(rew, rl, d, tr)
    if finish:
        ext.finish(obs)
    b = ext.batch()
    assert b.steps == k and (b.feat_tail is not None) == finish
    ended = (lens > 0) & (lens <= k)
    lens_eff = np.where(ended, lens, k)
    assert b.trunc.tolist() == np.where(ended, np.arange(N) & 1, 0).tolist()
    tr_stream = np.where(ended, (np.arange(N) & 1) == 1, True)
    assert (~ended).any() and (ended & (lens < k) & tr_stream).any() and (ended & ~tr_stream).any()
    tail = None
    if finish:  # the rows after step k - 1 are the twin's record k
        tail = b.feat_tail.reshape(-1, 13).cpu()
        nb = R["never"]["batch"]
        NS = N * nb.S
        twin_k = nb.obs_c_tm.reshape(T, NS, 13)[k].cpu()
        col = torch.arange(NS) if nb.rec_of is None else nb.rec_of.long().cpu()
        present = col >= 0
        assert same_bits(tail[present].numpy(), twin_k[col[present]].numpy())
    got = bucket_segments(b, status=ext.status, boot=critics())
    counts = check_bootstrap(B, case, got, bucket_segments(b), lens_eff, k, tr_stream, tail)
    assert all(nb > 0 for nb, nt in counts)
    if not finish:  # without finish only the streams that ended before k by a truncation are bootstrapped
        seg = np.repeat(ended & (lens < k) & tr_stream, b.S) & b.exist.reshape(-1).bool().cpu().numpy()
        assert sum(nb for nb, nt in counts) == int(seg.sum())


def test_collect_with_check_every_finishes():
    from mhppo.external import ExternalRollout
    from mhppo.rollout import bucket_segments, bucket_segments_ragged_torch
    case = ROLL[0]
    B = boot_runs(case)
    T = case[5]
    lens = 1 + (7 * np.arange(N)) % 9  # every stream ends, the last at step 9
    done = np.arange(T)[:, None] == lens[None, :] - 1
    ext = ExternalRollout(B["R"]["pol"], N, T=T, seed=SEED, early_end=True, bootstrap=True)
    sim = TruncSim(make_env(case), done, trunc_schedule(lens, T))
    b = ext.collect(sim, ITER, check_every=4)
    assert b.steps == 12 == sim.t and b.len.tolist() == lens.tolist() and b.trunc.tolist() == want_trunc(lens).tolist()
    assert b.feat_tail is not None  # finish ran on the rows of the step the loop broke at
    got = bucket_segments(b, status=ext.status, boot=critics())
    buckets_equal(got, bucket_segments_ragged_torch(b, boot=critics()))
    assert not eq(got[0]["ret"], bucket_segments(b)[0]["ret"])


# ------------------------------------------------------------------ 4. training
@pytest.mark.parametrize("opts", [{}, dict(gae_lambda=0.95)], ids=["plain", "gae"])
def test_train_external_bootstrap_equals_by_hand(opts):
    from mhppo.algo import Algo_PPO
    from mhppo.external import ExternalRollout
    from mhppo.models import Model_PPO
    from mhppo.rollout import bucket_segments_ragged_torch
    case = ("scalable", 4, 3, 2, 0, 20)
    T = case[5]
    lens, done = schedule(N, T)
    trunc = trunc_schedule(lens, T)
    torch.manual_seed(3)
    a = Algo_PPO(Model_PPO, make_env(case), seed=6, verbose=False, save_curves=False, **opts)
    b = Algo_PPO(Model_PPO, make_env(case), seed=6, verbose=False, save_curves=False, **opts)
    for na, nb in zip(a.nets(), b.nets()):
        nb.load_state_dict(na.state_dict())
    before = {k: v.clone() for k, v in algo_state(a).items()}
    sim_a, sim_b = TruncSim(make_env(case), done, trunc), TruncSim(make_env(case), done, trunc)
    a.train_external(sim_a, 2, M=N, early_end=True, bootstrap=True)
    assert a._external[0] == (N, T, True, True, True)  # both new arguments are part of the cache key
    assert a.rollout.batch.trunc.tolist() == want_trunc(lens).tolist() and a.rollout.batch.feat_tail is not None
    # the same two iterations by hand, on the torch specification of the bucketing
    r = b.rollout
    r.fix_bucket = b.fix_bucket
    lam = getattr(b, "gae_lambda", None)
    r.gae = None if lam is None else (b.critic_net_cross, b.critic_net_wait, b.gamma, lam)
    ext = ExternalRollout(b.policy(), N, T=T, early_end=True, bootstrap=True)
    ext.session.first_env = int(b.venv.cfg.env_id_offset)
    rets = []
    for ep in range(2):
        ext.session.seed = int(r.seed)
        r.batch = ext.collect(sim_b, r.iteration)
        r.iteration += 1
        r.cross, r.wait, r.choice = bucket_segments_ragged_torch(r.batch, fix_bucket=r.fix_bucket, status=ext.status,
                                                                 gae=r.gae, boot=(b.critic_net_cross, b.critic_net_wait))
        plain = bucket_segments_ragged_torch(r.batch, fix_bucket=r.fix_bucket, gae=r.gae)
        rets.append(not eq(plain[0]["ret"], r.cross["ret"]))
        b._after_collect(ep, reset_env=False)
    b._finish_train()
    assert all(rets)  # the bootstrap did change the targets
    sa, sb = algo_state(a), algo_state(b)
    assert set(sa) == set(sb) and any(k.startswith("opt.") and k.endswith("exp_avg") for k in sa)
    for k in sa:
        assert eq(sa[k], sb[k]), k
    assert any(not eq(sa[k], before[k]) for k in before if k.startswith("net"))
    ca, cb = a.curves(), b.curves()
    assert ca == cb and len(ca[2]) == 2
    # cut_truncates is part of the key; without bootstrap the key is the one it was
    a.train_external(TruncSim(make_env(case), done, trunc), 1, M=N, early_end=True, bootstrap=True, cut_truncates=False)
    assert a._external[0] == (N, T, True, True, False) and a.rollout.batch.cut_truncates is False
    a.train_external(ScheduledSim(make_env(case), done), 1, M=N, early_end=True)
    assert a._external[0] == (N, T, True) and getattr(a.rollout.batch, "trunc", None) is None
    with pytest.raises(ValueError):
        a.train_external(sim_a, 1, M=N, bootstrap=True)


# ------------------------------------------------------------------ 5. misuse
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
    with pytest.raises(ValueError):
        ExternalRollout(pol, M, T=T, bootstrap=True)  # bootstrap needs early_end
    plain = ExternalRollout(pol, M, T=T, early_end=True)
    assert plain.trunc is None
    plain.begin(obs, 0)
    plain.act(obs, 0)
    with pytest.raises(ValueError):
        plain.record(rew, rew, done, done)  # truncated without bootstrap
    plain.record(rew, rew, done)
    with pytest.raises(ValueError):
        plain.finish(obs)  # finish without bootstrap
    with pytest.raises(ValueError):
        bucket_segments(ExternalRollout(pol, M, T=1).collect(_OneStep(obs, rew), 0), boot=critics())  # not a ragged batch
    ext = ExternalRollout(pol, M, T=T, early_end=True, bootstrap=True)
    ext.begin(obs, 0)
    with pytest.raises(ValueError):
        ext.finish(obs)  # before any step is recorded
    ext.act(obs, 0)
    for bad in (None, done[:4], done.reshape(M, 1), done.cpu(), done.float(), done.int(), [False] * M):
        with pytest.raises(ValueError):
            ext.record(rew, rew, done, bad)
    ext.record(rew, rew, ~done, done.to(torch.uint8))  # every stream ends at step 0, none truncated
    assert ext.batch().feat_tail is None and ext.trunc.tolist() == [0] * M and ext.len.tolist() == [1] * M
    ext.finish(obs)
    with pytest.raises(ValueError):
        ext.finish(obs)  # twice
    ext.act(obs, 1)
    with pytest.raises(ValueError):
        ext.record(rew, rew, done, done)  # record after finish
    assert tuple(ext.batch().feat_tail.shape) == (M, S, 13)
    ext.begin(obs, 1)  # a new episode: the flags and the tail start again
    assert ext.trunc.tolist() == [0] * M and ext.feat_tail is None
    ext.act(obs, 0)
    ext.record(rew, rew, ~done, ~done)
    assert ext.trunc.tolist() == [1] * M


class _OneStep:
    """a one-step simulator for a fixed-length batch"""

    def __init__(self, obs, rew):
        self.obs, self.rew = obs, rew

    def reset(self):
        return self.obs

    def step(self, actions):
        return self.obs, self.rew, self.rew


def test_abi_rejects_bad_input():
    from mhppo import _lib
    from mhppo.models import Model_PPO
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    M, S, k = 4, 2, 3
    NS = M * S
    f = lambda n: torch.full((n,), SENT, dtype=torch.float32, device="cuda")
    c0, c1 = critics()
    d0, keep0 = c0.mlp_desc()
    d1, keep1 = c1.mlp_desc()
    actor = Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda()
    da, keepa = actor.mlp_desc()
    narrow = Model_PPO(12, 1, 0).cuda()
    dn, keepn = narrow.mlp_desc()
    a = dict(pos=torch.zeros(NS, dtype=torch.int64, device="cuda"), bucket=torch.zeros(NS, dtype=torch.int8, device="cuda"),
             len=torch.zeros(M, dtype=torch.int32, device="cuda"), trunc=torch.ones(M, dtype=torch.uint8, device="cuda"),
             obs=f(k * NS * 13), v=f(NS))

    def boot(c0=d0, c1=d1, M=M, S=S, k=k, **null):
        q = {key: (None if key in null else p(x)) for key, x in a.items()}
        return L.mhppo_boot_values(None if c0 is None else ctypes.byref(c0), None if c1 is None else ctypes.byref(c1),
                                   q["pos"], q["bucket"], None, q["len"], q["trunc"], M, S, k, 1, q["obs"], None, q["v"], st)

    bad = [boot(c0=None), boot(c1=None), boot(c0=da), boot(c1=da), boot(c1=dn), boot(M=-1), boot(S=0), boot(M=2**30, S=2),
           boot(k=0)]
    bad += [boot(**{key: 1}) for key in a]
    assert all(rc == -1 for rc in bad), bad
    assert b"boot_values" in L.mhppo_last_error()
    assert boot(M=0) == 0 and boot(M=0, pos=1, v=1) == 0  # M == 0 launches nothing, whatever the pointers
    # the scans
    rew = torch.full((k * NS,), SENT, dtype=torch.float64, device="cuda")
    ret, lrec = f(k * NS), torch.ones(NS, dtype=torch.int32, device="cuda")
    scan = lambda rew=rew, ret=ret, B=NS, T=k: L.mhppo_returns_scan_tm_boot(p(rew), p(ret), B, T, GAMMA, p(lrec), p(a["v"]), st)
    assert [scan(rew=None), scan(ret=None), scan(B=-1), scan(T=0)] == [-1] * 4 and scan(B=0) == 0
    assert L.mhppo_returns_scan_tm_boot(None, p(ret), NS, k, GAMMA, p(lrec), None, st) == -1  # the _len path's check
    gae = lambda T=k, obs=a["obs"], lam=0.9, lrec=lrec: L.mhppo_gae_tm_boot(
        ctypes.byref(d0), None, p(obs), p(rew), None, None, NS, T, GAMMA, lam, p(ret), None, p(lrec), p(a["v"]), st)
    assert gae(T=0) == -1 and gae(obs=None) == -1 and gae(lam=1.5) == -1
    assert gae(lrec=None) == -1 and b"len_rec" in L.mhppo_last_error()  # v_boot needs the lengths
    torch.cuda.synchronize()
    for x in (a["obs"], a["v"], ret, rew):
        assert bool((x == SENT).all())
