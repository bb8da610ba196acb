"""Early episode ends on the CPU: the torch specifications of the ragged bucketing (mhppo.rollout
.bucket_segments_ragged_torch, ragged_plan_torch, the len_rec forms of returns_scan_tm and gae_targets_torch)
and of the done-aware record step (mhppo.external.record_step_done_torch).  Every comparison is bit for bit:
  1. bucket_segments_ragged_torch against a plain per-segment numpy loop, in both record layouts;
  2. with no stream ended and k == T it is bucket_segments_torch;
  3. gae_targets_torch(len_rec=...) is the un-masked function applied to each truncated column;
  4. the wait rows start at a multiple of 4 when the cross rows do not end at one;
  5. record_step_done_torch freezes ep_min and keeps the first done; argument validation."""
import numpy as np
import pytest
import torch

KEYS = ("obs", "act", "logp", "ret", "rew")
GAMMA = 0.99


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def eq(a, b):
    return same_bits(a.numpy(), b.numpy())


def synthetic_batch(N, S, P, T, compact, seed, lens, k, dc=5):
    """A RolloutBatch of random records on the CPU.  Half of the segments exist; records of columns that
    hold none, and every record at or past its stream's length, are NaN: none may reach a bucket."""
    from mhppo.external import record_begin_torch
    from mhppo.rollout import RolloutBatch
    g = torch.Generator().manual_seed(seed)
    NS = N * S
    exist = (torch.rand((N, S), generator=g) < 0.6).to(torch.uint8)
    exist[0, 0] = 1
    a_d = (torch.rand((N, S, P), generator=g) < 0.5).to(torch.int32)
    closest = torch.randint(0, P, (N, S), generator=g, dtype=torch.int32)
    rec_of = record_begin_torch(exist, True)[1][:NS] if compact else None
    obs = torch.randn((T, NS, 13), generator=g)
    act, logp = torch.randn((T, NS), generator=g), torch.randn((T, NS), generator=g)
    rew = torch.randn((T, NS), generator=g, dtype=torch.float64)
    eff = [l if 0 < l <= k else k for l in lens]
    col_len = np.zeros(NS, dtype=np.int64)  # per record column
    for s in range(NS):
        c = s if rec_of is None else int(rec_of[s])
        if c >= 0:
            col_len[c] = eff[s // S]
    dead = torch.arange(T)[:, None] >= torch.from_numpy(col_len)[None, :]
    for x in (obs, act, logp, rew):
        x[dead] = float("nan")
    ep_min = -torch.rand((N, S), generator=g, dtype=torch.float64)
    return RolloutBatch(feat_d=torch.randn((N, S, P, dc), generator=g), logp_d=torch.randn((N, S, P), generator=g),
                        a_d=a_d, closest=closest, exist=exist, ep_min=ep_min, rec_of=rec_of, obs_c_tm=obs.reshape(T, N, S, 13),
                        act_tm=act.reshape(T, N, S), logp_tm=logp.reshape(T, N, S), rew_tm=rew.reshape(T, N, S),
                        N=N, S=S, P=P, T=T, len=torch.tensor(lens, dtype=torch.int32), steps=k), eff


def loop_buckets(b, eff, fix_bucket):
    """The ragged buckets by a plain loop over the segments in (stream, slot) order."""
    N, S, P, T = b.N, b.S, b.P, b.T
    NS = N * S
    a_d, closest, exist = b.a_d.numpy(), b.closest.numpy(), b.exist.numpy()
    recs = dict(obs=b.obs_c_tm.reshape(T, NS, 13).numpy(), act=b.act_tm.reshape(T, NS).numpy(),
                logp=b.logp_tm.reshape(T, NS).numpy(), rew=b.rew_tm.reshape(T, NS).numpy())
    out = [{k: [] for k in KEYS}, {k: [] for k in KEYS}]
    nseg = [0, 0]
    for n in range(N):
        for i in range(S):
            if not exist[n, i]:
                continue
            a = a_d[n, i, closest[n, i]] if fix_bucket else a_d[n].reshape(-1)[i]
            w = 1 if 2 * int(a) - 1 > 0 else 0
            s = n * S + i
            c = s if b.rec_of is None else int(b.rec_of[s])
            L = eff[n]
            ret, G = np.zeros(L, dtype=np.float32), 0.0
            for t in range(L - 1, -1, -1):
                G = recs["rew"][t, c] + GAMMA * G
                ret[t] = np.float32(G)
            for k in ("obs", "act", "logp", "rew"):
                out[w][k].append(recs[k][:L, c])
            out[w]["ret"].append(ret)
            nseg[w] += 1
    cat = lambda xs, like: np.concatenate(xs) if xs else like[:0, 0]
    return [{k: cat(o[k], recs[k] if k != "ret" else recs["act"]) for k in KEYS} for o in out], nseg


LENS = [3, 0, 1, 7, 9, 0, 2, 7, 5]  # 0: never ends; 7 == T; 9 > k counts as still running


@pytest.mark.parametrize("fix_bucket", [False, True], ids=["rule", "fix_bucket"])
@pytest.mark.parametrize("k", [7, 4])
@pytest.mark.parametrize("compact", [False, True], ids=["identity", "compact"])
def test_ragged_torch_equals_loop(compact, k, fix_bucket):
    from mhppo.rollout import bucket_segments, bucket_segments_ragged_torch
    N, S, P, T = len(LENS), 3, 2, 7
    b, eff = synthetic_batch(N, S, P, T, compact, 11, LENS, k)
    assert 1 in eff and k in eff and eff[4] == k
    plan = {}
    cross, wait, choice = bucket_segments_ragged_torch(b, fix_bucket=fix_bucket, plan_out=plan)
    want, nseg = loop_buckets(b, eff, fix_bucket)
    assert nseg[0] > 0 and nseg[1] > 0
    for name, got, w, n in (("cross", cross, want[0], nseg[0]), ("wait", wait, want[1], nseg[1])):
        assert got["n_seg"] == n and got["rows"] == w["act"].shape[0], name
        for key in KEYS:
            assert same_bits(got[key].numpy(), w[key]), (name, key)
            assert not bool(torch.isnan(got[key]).any()), (name, key)
    # the choice batch does not depend on the lengths; its ret is ep_min as it stands
    ex = b.exist.reshape(-1).bool()
    assert choice["n_seg"] == int(ex.sum()) == nseg[0] + nseg[1]
    assert eq(choice["ret"], b.ep_min.reshape(-1)[ex].float())
    sums = choice["rew_sums"].tolist()
    for i, w in enumerate(want):
        x = w["rew"].astype(np.float32).astype(np.float64)  # two summation orders of n terms
        assert abs(sums[i] - float(x.sum())) <= 2 * (x.size - 1) * 2.0 ** -53 * float(np.abs(x).sum()), i
    # bucket_segments dispatches on batch.len
    again = bucket_segments(b, fix_bucket=fix_bucket)
    assert again[0]["rows"] == cross["rows"] and eq(again[1]["ret"], wait["ret"])
    # the plan: contiguous segments, the wait rows aligned
    row0, len_rec, pos = plan["row0"], plan["len_rec"], plan["pos"]
    assert bool(((row0 >= 0) == (pos >= 0)).all()) and len_rec.dtype == torch.int32 and row0.dtype == torch.int64
    w0 = (cross["rows"] + 3) // 4 * 4
    used1 = (pos >= 0) & (plan["bucket"] != 0)
    assert int(row0[used1].min()) == w0 and int(row0[(pos >= 0) & (plan["bucket"] == 0)].min()) == 0


@pytest.mark.parametrize("compact", [False, True], ids=["identity", "compact"])
def test_no_early_end_is_the_fixed_length_path(compact):
    from mhppo.rollout import bucket_segments_ragged_torch, bucket_segments_torch
    N, S, P, T = 6, 2, 2, 5
    b, eff = synthetic_batch(N, S, P, T, compact, 5, [0] * N, T)
    assert eff == [T] * N
    rag = bucket_segments_ragged_torch(b)
    del b.__dict__["len"], b.__dict__["steps"]
    fix = bucket_segments_torch(b)
    for name, x, y in zip(("cross", "wait", "choice"), rag, fix):
        assert x["n_seg"] == y["n_seg"], name
        for key in y:
            if key != "n_seg":
                assert eq(x[key], y[key]), (name, key)
    assert rag[0]["rows"] == fix[0]["n_seg"] * T and rag[1]["rows"] == fix[1]["n_seg"] * T
    assert rag[0]["n_seg"] > 0 and rag[1]["n_seg"] > 0


def test_gae_len_is_the_truncated_scan():
    from mhppo.rollout import gae_targets_torch, returns_scan_tm
    T, B = 9, 12
    g = torch.Generator().manual_seed(3)
    rew = torch.randn((T, B), generator=g, dtype=torch.float64)
    v = torch.randn((T, B), generator=g)
    lens = torch.tensor([0, 1, 2, 9, 5, 9, 1, 3, 0, 8, 4, 9], dtype=torch.int32)
    bad = torch.arange(T)[:, None] >= lens[None, :]
    rew_n, v_n = rew.clone(), v.clone()
    rew_n[bad], v_n[bad] = float("nan"), float("nan")  # nothing past a length is read into a result
    for lam in (0.95, 1.0, 0.0):
        got = gae_targets_torch(rew_n, v_n, GAMMA, lam, len_rec=lens)
        got64 = gae_targets_torch(rew_n, v_n, GAMMA, lam, out_dtype=torch.float64, len_rec=lens)
        for b in range(B):
            L = int(lens[b])
            assert bool((got[L:, b] == 0).all()) and bool((got64[L:, b] == 0).all())
            if L:
                assert eq(got[:L, b], gae_targets_torch(rew[:L, b:b + 1], v[:L, b:b + 1], GAMMA, lam)[:, 0]), (lam, b)
    assert eq(gae_targets_torch(rew, v, GAMMA, 0.9, len_rec=torch.full((B,), T, dtype=torch.int32)),
              gae_targets_torch(rew, v, GAMMA, 0.9))
    # the reward-to-go scan likewise
    ret = returns_scan_tm(rew_n, GAMMA, len_rec=lens)
    for b in range(B):
        L = int(lens[b])
        assert bool((ret[L:, b] == 0).all())
        if L:
            assert eq(ret[:L, b], returns_scan_tm(rew[:L, b:b + 1].contiguous(), GAMMA)[:, 0])
    assert eq(returns_scan_tm(rew, GAMMA, len_rec=torch.full((B,), T, dtype=torch.int32)), returns_scan_tm(rew, GAMMA))


def test_plan_aligns_the_wait_rows():
    from mhppo.rollout import ragged_plan_torch
    M, S, k = 4, 2, 6
    pos = torch.tensor([0, 5, -1, 1, 4, 2, -1, 6])  # three cross, three wait (from w0 = 4), two unused
    bucket = torch.tensor([0, 1, 0, 0, 1, 0, 0, 1], dtype=torch.int8)
    ln = torch.tensor([2, 0, 3, 1], dtype=torch.int32)  # lengths 2, 6, 3, 1
    row0, len_rec, info = ragged_plan_torch(pos, bucket, None, ln, M, S, k)
    assert len_rec.tolist() == [2, 2, 6, 6, 3, 3, 1, 1]
    rows_cross, rows_wait = info.tolist()
    assert (rows_cross, rows_wait) == (2 + 6 + 3, 2 + 3 + 1) and rows_cross % 4 != 0
    w0 = (rows_cross + 3) // 4 * 4
    assert w0 % 4 == 0 and w0 == 12
    assert row0.tolist() == [0, w0, -1, 2, w0 + 2, 8, -1, w0 + 5]
    # the compact layout: column rec_of[s] takes segment s's stream's length, the rest 0
    rec_of = torch.tensor([0, -1, 1, 2, -1, -1, 3, 4], dtype=torch.int32)
    pos_c = torch.tensor([0, 1, 4, -1, 2, -1, -1, -1])
    bucket_c = torch.tensor([0, 0, 1, 0, 0, 0, 0, 0], dtype=torch.int8)
    row0, len_rec, info = ragged_plan_torch(pos_c, bucket_c, rec_of, ln, M, S, k)
    assert len_rec.tolist() == [2, 6, 6, 1, 1, 0, 0, 0]
    assert info.tolist() == [2 + 6 + 1, 6] and row0.tolist() == [0, 2, 12, -1, 8, -1, -1, -1]
    # nothing used, and nothing at all
    row0, len_rec, info = ragged_plan_torch(torch.full((8,), -1), bucket, None, ln, M, S, k)
    assert info.tolist() == [0, 0] and row0.tolist() == [-1] * 8
    row0, len_rec, info = ragged_plan_torch(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int8), None,
                                            torch.zeros(0, dtype=torch.int32), 0, S, k)
    assert info.tolist() == [0, 0] and row0.numel() == 0 and len_rec.numel() == 0


def test_record_step_done_spec():
    """ep_min freezes at the first done, len keeps it, a repeated done is ignored, the records are stored for
    finished streams too"""
    from mhppo.external import record_begin_torch, record_step_done_torch
    M, S, T = 4, 2, 4
    ep_min, _ = record_begin_torch(torch.ones((M, S), dtype=torch.uint8))
    ln = torch.zeros(M, dtype=torch.int32)
    recs = (torch.zeros((T, M * S, 13)), torch.zeros((T, M * S)), torch.zeros((T, M * S)),
            torch.zeros((T, M * S), dtype=torch.float64))
    dones = [[1, 0, 0, 0], [1, 1, 0, 0], [0, 1, 0, 0], [1, 0, 0, 1]]  # stream 0 at 0 (repeated), 1 at 1, 2 never, 3 at T - 1
    z = torch.zeros((M, S))
    for t in range(T):
        rl = torch.full((M, S), -float(t + 1), dtype=torch.float64)
        record_step_done_torch(t, z + t + 1, z, torch.zeros((M, S, 13)), rl.clone(), rl, None, *recs, ep_min,
                               torch.tensor(dones[t], dtype=torch.bool), ln)
    assert ln.tolist() == [1, 2, 0, 4]
    assert ep_min[:, 0].tolist() == [-1.0, -2.0, -4.0, -4.0]
    assert bool((recs[1] == (torch.arange(T) + 1.0)[:, None]).all())


def test_arguments_are_validated():
    from mhppo.rollout import (bucket_segments_ragged_torch, gae_targets_torch, ragged_plan_torch, returns_scan_tm)
    N, S, P, T = 3, 2, 1, 4
    b, _ = synthetic_batch(N, S, P, T, False, 1, [0, 2, 4], T)
    for bad in (dict(steps=0), dict(steps=T + 1), dict(len=b.len.long()), dict(len=b.len[:2]), dict(len=[0, 2, 4])):
        keep = dict(b.__dict__)
        b.__dict__.update(bad)
        with pytest.raises(ValueError):
            bucket_segments_ragged_torch(b)
        b.__dict__.update(keep)
    bucket_segments_ragged_torch(b)
    rew = torch.zeros((T, 5), dtype=torch.float64)
    for bad in (torch.zeros(5, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), [1] * 5):
        with pytest.raises(ValueError):
            returns_scan_tm(rew, GAMMA, len_rec=bad)
        with pytest.raises(ValueError):
            gae_targets_torch(rew, rew.float(), GAMMA, 0.9, len_rec=bad)
    with pytest.raises(ValueError):
        ragged_plan_torch(torch.zeros(6, dtype=torch.int64), torch.zeros(6, dtype=torch.int8), None, b.len, N, S, 0)
