"""The record pass's executable specification (mhppo.external.record_begin_torch / record_step_torch) on
the CPU: an oracle env driven by the host build of the sampling rule (tools/hostpolicy.py) on the rollout
fixtures' weights and recorded draws, every step recorded through the specification, must give
bucket_segments_torch the batches it makes of the oracle's own rollout records (oracle.OracleBatch.rollout)
for the same draws, bit for bit, in the identity and (scalable) the compact layout; and the specification's
edge cases: the NaN-propagating episodic minimum against a scalar restatement, rec_of of all-absent and
all-present rows, a single segment."""
import functools
import math
import os
import struct
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FIXTURES = ["rollout_coop_422", "rollout_naif_111", "rollout_scalable_422", "rollout_scalable_814"]
T = 80
KEYS = ("obs", "act", "logp", "ret", "rew")
CASES = [(n, False) for n in FIXTURES] + [(n, True) for n in FIXTURES if "scalable" in n]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def eq(a, b):
    return same_bits(a.numpy(), b.numpy())


def tm(x):
    """[n, S, T, ...] records -> time-major [T, n, S, ...]"""
    return torch.from_numpy(np.ascontiguousarray(np.moveaxis(x, 2, 0)))


@functools.lru_cache(maxsize=None)
def replay(name):
    """(the oracle's own rollout records, the rule's decision, per step the rule's records and the env's
    rewards) for a fixture's weights and draws"""
    import hostpolicy as hp
    import oracle
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    variant, shape = str(g["variant"]), (int(g["nb_car"]), int(g["nb_ped"]), int(g["nb_lines"]))
    eps, a_d, seed = g["eps"], g["a_d"], int(g["seed_base"])
    N = a_d.shape[0]
    c = hp.cfg(variant, *shape)
    w = [g["w_cross"], g["w_wait"], g["w_choice"]]
    ref = oracle.OracleBatch(variant, N, *shape, seed_base=seed).rollout(*w, forced_a=a_d, eps=eps, T=T)
    env = oracle.OracleBatch(variant, N, *shape, seed_base=seed)
    obs = env.reset()
    d = hp.sample_decide(c, w[2], obs, forced=a_d)
    steps = []
    for t in range(T):
        r = hp.sample_act(c, w[0], w[1], obs, a_d, d["closest"], eps=eps[t])
        obs, rew, rl, done = env.step(r["actions"])[:4]
        assert not done[:].any() or t == T - 1, "an episode ended before the time limit"
        steps.append((r["act"], r["logp"], r["feat_c"], rew, rl))
    return variant, ref, d, steps


def batch_of(d, recs, ep_min, rec_of, N, S, P):
    from mhppo.rollout import RolloutBatch
    t = torch.from_numpy
    return RolloutBatch(feat_d=t(d["feat_d"]), probs_d=t(d["probs_d"] if "probs_d" in d else d["probs"]),
                        logp_d=t(d["logp_d"]), a_d=t(d["a_d"]), closest=t(d["closest"]), exist=t(d["exist"]),
                        obs_c_tm=recs[0], act_tm=recs[1], logp_tm=recs[2], rew_tm=recs[3], ep_min=ep_min, rec_of=rec_of,
                        N=N, S=S, P=P, T=T)


@functools.lru_cache(maxsize=None)
def buckets(name, compact):
    """(the specification's buckets, the oracle records' buckets) of a fixture, with the checks on the way"""
    from mhppo.external import record_begin_torch, record_step_torch
    from mhppo.rollout import bucket_segments_torch
    variant, ref, d, steps = replay(name)
    N, S, P = ref["a_d"].shape
    exist = torch.from_numpy(d["exist"])
    if variant == "scalable":
        assert bool((exist == 0).any()) and bool((exist != 0).any())
    NS = N * S
    ep_min, rec = record_begin_torch(exist, compact)
    rec_of = rec[:NS] if compact else None
    recs = (torch.full((T, NS, 13), -7.0), torch.full((T, NS), -7.0), torch.full((T, NS), -7.0),
            torch.full((T, NS), -7.0, dtype=torch.float64))
    for t, (act, logp, feat_c, rew, rl) in enumerate(steps):
        f = torch.from_numpy
        record_step_torch(t, f(act), f(logp), f(feat_c), f(rew), f(rl), rec_of, *recs, ep_min)
    assert same_bits(ep_min.numpy(), ref["ep_min"])
    if compact:  # nothing stored past the present segments' records
        n_rec = int(rec[NS + N])
        assert n_rec == int((exist != 0).sum()) and bool((recs[1][:, n_rec:] == -7.0).all())
        assert bool((recs[1][:, :n_rec] != -7.0).any())
    # the oracle's logp_d is its own logf's; the rule's is compared with it in tests/test_policy_sample_host.py
    # and is not the record pass's business: both batches carry the oracle's
    dd = dict(d, logp_d=ref["logp_d"])
    for k in ("a_d", "feat_d", "closest", "exist"):
        assert same_bits(dd[k], ref[k]), k
    got = bucket_segments_torch(batch_of(dd, recs, ep_min, rec_of, N, S, P))
    o_recs = (tm(ref["obs_c"]).reshape(T, NS, 13), tm(ref["act"]).reshape(T, NS), tm(ref["logp"]).reshape(T, NS),
              tm(ref["rew"]).reshape(T, NS))
    want = bucket_segments_torch(batch_of(ref, o_recs, torch.from_numpy(ref["ep_min"]), None, N, S, P))
    return got, want, int((exist != 0).sum())


@pytest.mark.parametrize("name,compact", CASES, ids=lambda v: v if isinstance(v, str) else ("identity", "compact")[v])
def test_spec_replays_oracle_buckets(name, compact):
    got, want, n_present = buckets(name, compact)
    for b, (x, y) in zip(("cross", "wait", "choice"), zip(got, want)):
        assert x["n_seg"] == y["n_seg"], b
        for k in KEYS:
            if k in y:
                assert eq(x[k], y[k]), (b, k)
    assert got[0]["n_seg"] + got[1]["n_seg"] == got[2]["n_seg"] == n_present
    assert got[0]["obs"].shape[0] == got[0]["n_seg"] * T


def test_both_buckets_non_empty_somewhere():
    """the cross and the wait bucket are both non-empty in at least one fixture"""
    sizes = {n: tuple(b["n_seg"] for b in buckets(n, False)[0][:2]) for n in FIXTURES}
    assert any(c > 0 and w > 0 for c, w in sizes.values()), sizes


def scalar_min(m, x):
    return m if m != m else (x if x != x else (x if x < m else m))


def f64_bits(v):
    return struct.pack("<d", v)


def test_minimum_nan_smaller_and_signed_zero():
    """ep_min over sequences with NaN, then a smaller value, then -0.0, against the scalar expression
    (of +0.0 and -0.0 the old value stays, whichever it is: x < m is false)."""
    from mhppo.external import record_begin_torch, record_step_torch
    nan = float("nan")
    seqs = [[nan, -1.0, -0.0], [0.5, nan, -2.0], [-0.0, 0.0, -0.0], [1.0, 2.0, -0.0], [-1.0, nan, -0.0],
            [-3.0, -5.0, -0.0], [0.0, -0.0, nan], [-0.0, -1e-300, 5.0]]
    M, S, TT = len(seqs), 1, 3
    ep_min, rec = record_begin_torch(torch.ones((M, S), dtype=torch.uint8))
    assert rec is None and all(f64_bits(v) == f64_bits(0.0) for v in ep_min.reshape(-1).tolist())
    recs = (torch.zeros((TT, M, 13)), torch.zeros((TT, M)), torch.zeros((TT, M)), torch.zeros((TT, M), dtype=torch.float64))
    want = [0.0] * M
    z = torch.zeros((M, S))
    for t in range(TT):
        x = torch.tensor([s[t] for s in seqs], dtype=torch.float64).reshape(M, S)
        record_step_torch(t, z, z, torch.zeros((M, S, 13)), x.clone(), x, None, *recs, ep_min)
        want = [scalar_min(m, s[t]) for m, s in zip(want, seqs)]
        for got, w in zip(ep_min.reshape(-1).tolist(), want):
            assert f64_bits(got) == f64_bits(w) or (math.isnan(got) and math.isnan(w)), (t, got, w)
        assert same_bits(recs[3][t].numpy(), x.reshape(-1).numpy())
    assert math.isnan(want[0]) and want[1] != want[1] and f64_bits(want[2]) == f64_bits(0.0)
    assert f64_bits(want[3]) == f64_bits(0.0)  # -0.0 < +0.0 is false: the old +0.0 stays
    with pytest.raises(ValueError):
        record_step_torch(TT, z, z, torch.zeros((M, S, 13)), z.double(), z.double(), None, *recs, ep_min)


def test_rec_of_all_absent_all_present_and_single():
    from mhppo.external import record_begin_torch, record_step_torch
    M, S = 5, 3
    ep, rec = record_begin_torch(torch.zeros((M, S), dtype=torch.uint8), compact=True)
    assert rec.dtype == torch.int32 and rec.tolist() == [-1] * (M * S) + [0] * (M + 1)
    ep, rec = record_begin_torch(torch.ones((M, S), dtype=torch.uint8), compact=True)
    assert rec.tolist() == list(range(M * S)) + [S * r for r in range(M + 1)]
    ex = torch.tensor([[1, 0, 1], [0, 0, 0], [0, 1, 1]], dtype=torch.uint8)
    ep, rec = record_begin_torch(ex, compact=True)
    assert rec.tolist() == [0, -1, 1, -1, -1, -1, -1, 2, 3] + [0, 2, 2, 4]
    # all absent: a step stores nothing and still takes the minimum
    ep, rec = record_begin_torch(torch.zeros((2, 2), dtype=torch.uint8), compact=True)
    recs = (torch.full((1, 4, 13), -7.0), torch.full((1, 4), -7.0), torch.full((1, 4), -7.0),
            torch.full((1, 4), -7.0, dtype=torch.float64))
    x = torch.tensor([[-1.0, 2.0], [float("nan"), -0.0]], dtype=torch.float64)
    record_step_torch(0, torch.ones(2, 2), torch.ones(2, 2), torch.ones(2, 2, 13), x, x, rec[:4], *recs, ep)
    assert all(bool((r == -7.0).all()) for r in recs)
    assert ep[0].tolist() == [-1.0, 0.0] and math.isnan(float(ep[1, 0])) and f64_bits(float(ep[1, 1])) == f64_bits(0.0)
    # M S = 1, both layouts
    for compact in (False, True):
        ep, rec = record_begin_torch(torch.ones((1, 1), dtype=torch.uint8), compact)
        assert (rec is None) if not compact else rec.tolist() == [0, 0, 1]
        recs = (torch.zeros((2, 1, 13)), torch.zeros((2, 1)), torch.zeros((2, 1)), torch.zeros((2, 1), dtype=torch.float64))
        feat = torch.arange(13.0).reshape(1, 1, 13)
        record_step_torch(1, torch.tensor([[3.0]]), torch.tensor([[-4.0]]), feat, torch.tensor([[5.0]], dtype=torch.float64),
                          torch.tensor([[-6.0]], dtype=torch.float64), None if rec is None else rec[:1], *recs, ep)
        assert recs[0][1, 0].tolist() == list(range(13)) and float(recs[1][1, 0]) == 3.0 and float(recs[2][1, 0]) == -4.0
        assert float(recs[3][1, 0]) == 5.0 and float(ep[0, 0]) == -6.0 and bool((recs[0][0] == 0).all())
    ep, rec = record_begin_torch(torch.zeros((0, 2), dtype=torch.uint8), compact=True)
    assert ep.shape == (0, 2) and rec.tolist() == [0]
