"""Truncation bootstrap on the CPU: the torch specifications (mhppo.rollout.boot_values_torch, the v_boot forms
of returns_scan_tm and gae_targets_torch, bucket_segments_ragged_torch(boot=...)) and the trunc update of
mhppo.external.record_step_done_torch.  Bit for bit unless a bound is named:
  1. boot_values_torch and the bootstrapped buckets against a plain per-segment numpy loop, in both record
     layouts, at k == T and k < T, with NaN in every record row and tail row the rule must not select;
  2. v_boot = 0 everywhere, or no truncation at all, is the len_rec form;
  3. ret[L - 1] == float32(rew[L - 1] + gamma float64(v_boot)), exactly;
  4. GAE at lambda = 1 with bootstrap is the bootstrapped reward-to-go within 1 float32 ulp, the bound
     tests/test_gae_host.py has for that identity without bootstrap (two float64 recurrences that differ by
     about T 2^-53 (|G| + |V|) differ after the cast only at a rounding boundary);
  5. record_step_done_torch reads truncated at the first done only; argument validation."""
import functools

import numpy as np
import pytest
import torch

from test_early_end_host import GAMMA, KEYS, eq, same_bits, synthetic_batch
from test_gae_host import _ulp_apart

T = 7
LENS = [3, 0, 1, 7, 9, 0, 2, 7, 5, 4, 4]   # 0: never ends; 7 == T; 9 > k counts as still running
TRUNC = [1, 1, 0, 1, 0, 0, 1, 0, 1, 0, 1]  # stream 1 never ends: its flag is never read
N, S, P = len(LENS), 3, 2


@functools.lru_cache(maxsize=None)
def critics():
    from mhppo.models import Model_PPO
    torch.manual_seed(5)
    return Model_PPO(13, 1, 0), Model_PPO(13, 1, 0)


def rule(b, k, cut, tail):
    """The rule of include/mhppo.h per segment, by a plain loop: (col, selected, bucket, L, successor row
    source) for every segment; None for segments without a record."""
    a_d, exist = b.a_d.numpy(), b.exist.numpy()
    out = []
    for n in range(N):
        for i in range(S):
            s = n * S + i
            col = s if b.rec_of is None else int(b.rec_of[s])
            if col < 0:
                out.append(None)
                continue
            ended = 1 <= LENS[n] <= k
            L = LENS[n] if ended else k
            tr = bool(TRUNC[n]) if ended else bool(cut)
            used = bool(exist[n, i])
            w = 1 if 2 * int(a_d[n].reshape(-1)[i]) - 1 > 0 else 0
            out.append(dict(s=s, col=col, L=L, w=w, used=used, sel=used and tr and (L < k or tail)))
    return out


def boot_batch(compact, k, cut, tail, seed=11):
    """synthetic_batch (every record at or past a stream's length NaN) with the truncation state: finite
    successor rows exactly where the rule selects one, NaN in every other tail row."""
    b, eff = synthetic_batch(N, S, P, T, compact, seed, LENS, k)
    g = torch.Generator().manual_seed(seed + 1)
    obs = b.obs_c_tm.reshape(T, N * S, 13)
    feat_tail = torch.full((N, S, 13), float("nan"))
    segs = rule(b, k, cut, tail)
    for x in segs:
        if x is None or not x["sel"]:
            continue
        row = torch.randn(13, generator=g)
        if x["L"] < k:
            assert bool(torch.isnan(obs[x["L"], x["col"]]).all())  # it was dead: only the rule's row becomes finite
            obs[x["L"], x["col"]] = row
        else:
            feat_tail.reshape(N * S, 13)[x["s"]] = row
    b.__dict__.update(trunc=torch.tensor(TRUNC, dtype=torch.uint8), feat_tail=feat_tail if tail else None,
                      cut_truncates=cut)
    return b, eff, segs


def loop_v_boot(b, segs, k):
    """v_boot per record column by the loop; V of the selected rows from ONE forward per critic over a
    [NS, 13] matrix, zero rows elsewhere -- the call the specification makes, so equal rows give equal bits."""
    NS = N * S
    obs = b.obs_c_tm.reshape(T, NS, 13)
    rows = torch.zeros((NS, 13))
    for x in segs:
        if x is not None and x["sel"]:
            rows[x["s"]] = obs[x["L"], x["col"]] if x["L"] < k else b.feat_tail.reshape(NS, 13)[x["s"]]
    assert not bool(torch.isnan(rows).any())
    with torch.no_grad():
        V = [c(rows).reshape(-1).numpy() for c in critics()]
    v = np.zeros(NS, dtype=np.float32)
    for x in segs:
        if x is not None and x["sel"]:
            v[x["col"]] = V[x["w"]][x["s"]]
    return v


def loop_buckets(b, segs, v_boot):
    """The ragged buckets' ret by a plain loop, every segment's scan started from its column's v_boot."""
    rew = b.rew_tm.reshape(T, N * S).numpy()
    out = [[], []]
    for x in segs:
        if x is None or not x["used"]:
            continue
        G, ret = float(np.float64(v_boot[x["col"]])), np.zeros(x["L"], dtype=np.float32)
        for t in range(x["L"] - 1, -1, -1):
            G = rew[t, x["col"]] + GAMMA * G
            ret[t] = np.float32(G)
        out[x["w"]].append(ret)
    return [np.concatenate(o) for o in out]


CASES = [(7, True, True), (7, True, False), (7, False, True), (4, True, True), (4, False, False)]


@pytest.mark.parametrize("k,cut,tail", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("compact", [False, True], ids=["identity", "compact"])
def test_boot_torch_equals_loop(compact, k, cut, tail):
    from mhppo.rollout import boot_values_torch, bucket_segments, bucket_segments_ragged_torch
    b, eff, segs = boot_batch(compact, k, cut, tail)
    c0, c1 = critics()
    plan = {}
    plain = bucket_segments_ragged_torch(b, plan_out=plan)
    assert "v_boot" not in plan
    got_v = boot_values_torch(c0, c1, plan["pos"], plan["bucket"], b.rec_of, b.len, b.trunc, N, S, k, cut, b.obs_c_tm,
                              b.feat_tail)
    want_v = loop_v_boot(b, segs, k)
    assert got_v.dtype == torch.float32 and same_bits(got_v.numpy(), want_v)
    sel = [x for x in segs if x is not None and x["sel"]]
    assert any(x["L"] < k for x in sel) and any(x["w"] == 0 for x in sel) and any(x["w"] == 1 for x in sel)
    assert any(x["L"] == k for x in sel) == tail  # with a tail some segment of length k is truncated in every case
    assert all(want_v[x["col"]] != 0 for x in sel) and np.count_nonzero(want_v) == len(sel)
    # the buckets: ret from the loop, every other key and the choice batch as without boot
    plan_b = {}
    boot = bucket_segments_ragged_torch(b, boot=(c0, c1), plan_out=plan_b)
    assert eq(plan_b["v_boot"], got_v)
    want = loop_buckets(b, segs, want_v)
    for i in range(2):
        assert same_bits(boot[i]["ret"].numpy(), want[i]), i
        assert not bool(torch.isnan(boot[i]["ret"]).any())
        assert not eq(boot[i]["ret"], plain[i]["ret"])
        for key in KEYS:
            if key != "ret":
                assert eq(boot[i][key], plain[i][key]), (i, key)
        assert boot[i]["rows"] == plain[i]["rows"] and boot[i]["n_seg"] == plain[i]["n_seg"]
    for key in plain[2]:
        assert boot[2][key] == plain[2][key] if key == "n_seg" else eq(boot[2][key], plain[2][key]), key
    again = bucket_segments(b, boot=(c0, c1))  # bucket_segments forwards boot
    assert eq(again[0]["ret"], boot[0]["ret"]) and eq(again[1]["ret"], boot[1]["ret"])


@pytest.mark.parametrize("compact", [False, True], ids=["identity", "compact"])
def test_gae_buckets_with_boot_equal_loop(compact):
    """GAE under boot: the recurrence of every used column by a numpy loop, V from the forward the
    specification makes over all records"""
    from mhppo.rollout import bucket_segments_ragged_torch
    k, lam = 4, 0.95
    b, eff, segs = boot_batch(compact, k, True, True)
    c0, c1 = critics()
    got = bucket_segments_ragged_torch(b, gae=(c0, c1, GAMMA, lam), boot=(c0, c1))
    v_boot = loop_v_boot(b, segs, k)
    NS = N * S
    with torch.no_grad():
        V = [c(b.obs_c_tm.reshape(T * NS, 13)).reshape(T, NS).numpy() for c in (c0, c1)]
    rew = b.rew_tm.reshape(T, NS).numpy()
    want = [[], []]
    for x in segs:
        if x is None or not x["used"]:
            continue
        A, nv, ret = 0.0, float(np.float64(v_boot[x["col"]])), np.zeros(x["L"], dtype=np.float32)
        for t in range(x["L"] - 1, -1, -1):
            v = float(np.float64(V[x["w"]][t, x["col"]]))
            d = (rew[t, x["col"]] + GAMMA * nv) - v
            A = d + (GAMMA * lam) * A
            ret[t] = np.float32(A + v)
            nv = v
        want[x["w"]].append(ret)
    for i in range(2):
        assert same_bits(got[i]["ret"].numpy(), np.concatenate(want[i])), i


@pytest.mark.parametrize("compact", [False, True], ids=["identity", "compact"])
def test_no_truncation_is_the_early_end_path(compact):
    from mhppo.rollout import bucket_segments_ragged_torch, gae_targets_torch, returns_scan_tm
    c0, c1 = critics()
    for k in (7, 4):
        b, eff, segs = boot_batch(compact, k, False, True)
        plain = bucket_segments_ragged_torch(b)
        b.trunc = torch.zeros(N, dtype=torch.uint8)  # no truncated flag raised, and the cut is terminal
        plan = {}
        for gae in (None, (c0, c1, GAMMA, 0.95)):
            base = plain if gae is None else bucket_segments_ragged_torch(b, gae=gae)
            boot = bucket_segments_ragged_torch(b, gae=gae, boot=(c0, c1), plan_out=plan)
            assert not bool(plan["v_boot"].any())
            for x, y in zip(boot, base):
                assert set(x) == set(y)
                for key in y:
                    assert x[key] == y[key] if key in ("n_seg", "rows") else eq(x[key], y[key]), key
        # boot on a batch without the truncation flags is not a bootstrap
        del b.__dict__["trunc"]
        none = bucket_segments_ragged_torch(b, boot=(c0, c1))
        assert eq(none[0]["ret"], plain[0]["ret"]) and eq(none[1]["ret"], plain[1]["ret"])
    # the scans with v_boot = 0
    g = torch.Generator().manual_seed(3)
    B = 12
    rew = torch.randn((T, B), generator=g, dtype=torch.float64)
    v = torch.randn((T, B), generator=g)
    lens = torch.tensor([0, 1, 2, 7, 5, 7, 1, 3, 0, 6, 4, 7], dtype=torch.int32)
    z = torch.zeros(B)
    assert eq(returns_scan_tm(rew, GAMMA, len_rec=lens, v_boot=z), returns_scan_tm(rew, GAMMA, len_rec=lens))
    assert eq(returns_scan_tm(rew, GAMMA, v_boot=z), returns_scan_tm(rew, GAMMA))
    for lam in (0.95, 1.0, 0.0):
        assert eq(gae_targets_torch(rew, v, GAMMA, lam, len_rec=lens, v_boot=z),
                  gae_targets_torch(rew, v, GAMMA, lam, len_rec=lens))


def scan_case(Tn, B, seed):
    g = torch.Generator().manual_seed(seed)
    rew = torch.randn((Tn, B), generator=g, dtype=torch.float64)
    v = torch.randn((Tn, B), generator=g)
    lens = torch.randint(0, Tn + 1, (B,), generator=g, dtype=torch.int32)
    lens[0], lens[1], lens[2] = Tn, min(1, Tn), 0
    vb = torch.randn(B, generator=g) * 3.0  # mixed sign
    bad = torch.arange(Tn)[:, None] >= lens[None, :]
    rew_n, v_n = rew.clone(), v.clone()
    rew_n[bad], v_n[bad] = float("nan"), float("nan")  # nothing at or past a length is read into a result
    return rew, v, rew_n, v_n, lens, vb


@pytest.mark.parametrize("Tn", (1, 7, 80))
def test_scans_with_v_boot(Tn):
    from mhppo.rollout import gae_targets_torch, returns_scan_tm
    B = 9
    rew, v, rew_n, v_n, lens, vb = scan_case(Tn, B, 40 + Tn)
    assert bool((vb > 0).any()) and bool((vb < 0).any()) and float(vb[2]) != 0.0
    ret = returns_scan_tm(rew_n, GAMMA, len_rec=lens, v_boot=vb)
    r, vbn = rew.numpy(), vb.numpy()
    for b in range(B):
        L = int(lens[b])
        assert bool((ret[L:, b] == 0).all())  # a column of no steps is all zeros whatever its v_boot
        G, want = float(np.float64(vbn[b])), np.zeros(L, dtype=np.float32)
        for t in range(L - 1, -1, -1):
            G = r[t, b] + GAMMA * G
            want[t] = np.float32(G)
        assert same_bits(ret[:L, b].numpy(), want), b
        if L:  # the last step, exactly
            assert ret[L - 1, b].item() == np.float32(r[L - 1, b] + GAMMA * np.float64(vbn[b]))
    # without lengths every column has Tn steps
    full = returns_scan_tm(rew, GAMMA, v_boot=vb)
    assert eq(full, returns_scan_tm(rew, GAMMA, len_rec=torch.full((B,), Tn, dtype=torch.int32), v_boot=vb))
    assert same_bits(full[Tn - 1].numpy(), (r[Tn - 1] + GAMMA * vbn.astype(np.float64)).astype(np.float32))
    # GAE: the float64 recurrence of include/mhppo.h by a loop
    for lam in (0.95, 1.0, 0.0):
        got = gae_targets_torch(rew_n, v_n, GAMMA, lam, len_rec=lens, v_boot=vb)
        for b in range(B):
            L = int(lens[b])
            assert bool((got[L:, b] == 0).all())
            A, nv, want = 0.0, float(np.float64(vbn[b])), np.zeros(L, dtype=np.float32)
            for t in range(L - 1, -1, -1):
                vt = float(np.float64(v[t, b].item()))
                d = (r[t, b] + GAMMA * nv) - vt
                A = d + (GAMMA * lam) * A
                want[t] = np.float32(A + vt)
                nv = vt
            assert same_bits(got[:L, b].numpy(), want), (lam, b)
    # lambda = 1 is the bootstrapped reward-to-go: the bound of tests/test_gae_host.py for the identity
    got = gae_targets_torch(rew_n, v_n, GAMMA, 1.0, len_rec=lens, v_boot=vb)
    live = ~(torch.arange(Tn)[:, None] >= lens[None, :])
    assert np.all(_ulp_apart(got[live].numpy(), ret[live].numpy()) <= 1.0)


def test_record_step_done_spec_keeps_the_first_truncated():
    from mhppo.external import record_begin_torch, record_step_done_torch
    M, S_, Tn = 5, 2, 4
    ep_min, _ = record_begin_torch(torch.ones((M, S_), dtype=torch.uint8))
    ln, trunc = torch.zeros(M, dtype=torch.int32), torch.zeros(M, dtype=torch.uint8)
    recs = (torch.zeros((Tn, M * S_, 13)), torch.zeros((Tn, M * S_)), torch.zeros((Tn, M * S_)),
            torch.zeros((Tn, M * S_), dtype=torch.float64))
    # stream 0: done at 0 with truncated, flags dropped later; 1: truncated raised before its done at 1, which is
    # terminal, and raised again after it; 2: never done, truncated raised alone; 3: done at T - 1, truncated;
    # 4: done twice, truncated only at the second
    dones = [[1, 0, 0, 0, 0], [1, 1, 0, 0, 1], [0, 1, 0, 0, 1], [1, 0, 0, 1, 0]]
    truncs = [[1, 1, 1, 0, 0], [0, 0, 1, 0, 0], [0, 1, 1, 0, 1], [0, 1, 0, 7, 1]]
    z = torch.zeros((M, S_))
    for t in range(Tn):
        rl = torch.full((M, S_), -float(t + 1), dtype=torch.float64)
        record_step_done_torch(t, z, z, torch.zeros((M, S_, 13)), rl.clone(), rl, None, *recs, ep_min,
                               torch.tensor(dones[t], dtype=torch.bool), ln, torch.tensor(truncs[t], dtype=torch.uint8),
                               trunc)
    assert ln.tolist() == [1, 2, 0, 4, 2]
    assert trunc.tolist() == [1, 0, 0, 1, 0] and trunc.dtype == torch.uint8
    with pytest.raises(ValueError):
        record_step_done_torch(0, z, z, torch.zeros((M, S_, 13)), rl, rl, None, *recs, ep_min,
                               torch.zeros(M, dtype=torch.bool), ln, torch.zeros(M, dtype=torch.uint8), None)


def test_arguments_are_validated():
    from mhppo.rollout import (boot_values_torch, bucket_segments, bucket_segments_ragged_torch, gae_targets_torch,
                               returns_scan_tm)
    c0, c1 = critics()
    b, eff, segs = boot_batch(False, T, True, True)
    plan = {}
    bucket_segments_ragged_torch(b, plan_out=plan)
    NS = N * S
    good = dict(pos=plan["pos"], bucket=plan["bucket"], rec_of=None, len=b.len, trunc=b.trunc, M=N, S=S, k=T,
                cut_truncates=True, obs_tm=b.obs_c_tm, feat_tail=b.feat_tail)
    boot_values_torch(c0, c1, **good)
    for bad in (dict(k=0), dict(pos=plan["pos"].int()), dict(pos=plan["pos"][:-1]), dict(bucket=plan["bucket"].long()),
                dict(len=b.len.long()), dict(trunc=b.trunc.bool()), dict(trunc=b.trunc[:-1]),
                dict(rec_of=torch.zeros(NS, dtype=torch.int64)), dict(obs_tm=b.obs_c_tm.double()),
                dict(obs_tm=b.obs_c_tm[:, :, :, :12]), dict(k=T + 1), dict(feat_tail=b.feat_tail[:-1]),
                dict(feat_tail=b.feat_tail.double())):
        with pytest.raises(ValueError):
            boot_values_torch(c0, c1, **{**good, **bad})
    rew = torch.zeros((T, 5), dtype=torch.float64)
    ln = torch.ones(5, dtype=torch.int32)
    for bad in (torch.zeros(5, dtype=torch.float64), torch.zeros(4), [0.0] * 5):
        with pytest.raises(ValueError):
            returns_scan_tm(rew, GAMMA, len_rec=ln, v_boot=bad)
        with pytest.raises(ValueError):
            gae_targets_torch(rew, rew.float(), GAMMA, 0.9, len_rec=ln, v_boot=bad)
    with pytest.raises(ValueError):
        gae_targets_torch(rew, rew.float(), GAMMA, 0.9, v_boot=torch.zeros(5))  # v_boot needs len_rec
    # boot is for ragged batches only
    del b.__dict__["len"], b.__dict__["steps"]
    with pytest.raises(ValueError):
        bucket_segments(b, boot=(c0, c1))
