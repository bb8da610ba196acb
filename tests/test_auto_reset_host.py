"""Auto-reset lanes on the CPU: the torch specifications of the lane bookkeeping (mhppo.external
.lanes_begin_torch / lanes_restart_torch / lanes_record_torch / lanes_close_torch) and of the lanes bucketing
(mhppo.rollout.returns_scan_tm_lanes_torch, bucket_segments_lanes_torch) against an independent numpy oracle
that walks each stream's done tape and splits it into episodes.  Everything is bit for bit except the reward
sums against a plain sum, which have the bound of two summation orders.
  1. the schedule contains every case: a done at t = 0, dones on consecutive steps, a done at the last
     recorded step (no empty lane), a stream that hits the cap E and idles, a stream that never ends;
  2. the four bookkeeping specifications driven over the tape: t0, len, cut, the per-lane ep_min and the
     lane decisions;
  3. bucket_segments_lanes_torch: the bucket rows in lane-segment order, the choice batch, the reward sums;
  4. the cut bootstrap: a cut lane's last target is (float)(rew + gamma (double)v_boot), an ended lane's
     (float)rew."""
import types

import numpy as np
import pytest
import torch

from test_early_end_gpu import schedule
from test_early_end_host import same_bits

KEYS = ("obs", "act", "logp", "ret", "rew")
GAMMA = 0.99
M, T = 23, 7
DEC = ("a_d", "logp_d", "probs", "feat_d", "closest", "exist")


def eq(a, b):
    return same_bits(a.numpy(), b.numpy())


def split(done, E, k):
    """The oracle: per stream the episodes [(t0, len, cut)] its done tape gives in k recorded steps under the
    cap E, and the steps at which it idles.  A lane exists once a step of it is acted on."""
    lanes, idle = [], []
    for r in range(done.shape[1]):
        eps, t0, n_idle = [], 0, 0
        for t in range(k):
            if t0 is None:
                if len(eps) == E:
                    n_idle += 1
                    continue
                t0 = t  # act(t) opens the next lane
            if done[t, r]:
                eps.append((t0, t + 1 - t0, 0))
                t0 = None
        if t0 is not None:
            eps.append((t0, k - t0, 1))
        lanes.append(eps)
        idle.append(n_idle)
    return lanes, idle


def check_split(done, E, k):
    """what the tests rely on the schedule to contain, at the cap E and k recorded steps"""
    lanes, idle = split(done, E, k)
    assert any(e[0][1] == 1 and not e[0][2] for e in lanes)  # a done at t = 0
    assert any(len(e) == 1 and e[0] == (0, k, 1) for e in lanes)  # never ends: one lane, cut at k
    if E >= 3:
        assert any(e[1][1] == 1 and not e[1][2] for e in lanes if len(e) > 1)  # dones on consecutive steps
    # a done at the last recorded step with a lane left: no empty lane is opened.  At E = 3, k = T the dones at
    # T - 1 are third ends (the cap; asserted below); k = 4 and E = 4 have the case with a lane to spare.
    last = [r for r, e in enumerate(lanes) if done[k - 1, r] and not e[-1][2] and sum(x[1] for x in e) == k and len(e) < E]
    if (E, k) in ((3, 4), (4, T)):
        assert last
    if (E, k) == (3, T):
        assert any(len(e) == E and n > 0 for e, n in zip(lanes, idle))  # hits the cap and idles
        assert any(len(e) == E and n == 0 and not e[-1][2] for e, n in zip(lanes, idle))  # the E-th end is the window's
    for e in lanes:
        assert 1 <= len(e) <= E and all(L >= 1 for _, L, _ in e)
        assert all(a[0] + a[1] == b[0] for a, b in zip(e, e[1:]))  # back to back: same-step auto-reset
    return lanes


def np_min(m, x):
    """mhppo_record_step's minimum"""
    return m if m != m else (x if x != x else (x if x < m else m))


def tape(S, P, seed, dc=5):
    """done [T, M] and T + 1 decisions / T steps of random inputs: NaN and -0.0 in rew_light"""
    g = torch.Generator().manual_seed(seed)
    _, done = schedule(M, T)
    decs = []
    for t in range(T):
        exist = (torch.rand((M, S), generator=g) < 0.7).to(torch.uint8)
        decs.append(types.SimpleNamespace(
            a_d=(torch.rand((M, S, P), generator=g) < 0.5).to(torch.int32), logp_d=torch.randn((M, S, P), generator=g),
            probs=torch.rand((M, S, P, 2), generator=g), feat_d=torch.randn((M, S, P, dc), generator=g),
            closest=torch.randint(0, P, (M, S), generator=g, dtype=torch.int32), exist=exist))
    steps = []
    for t in range(T):
        rl = -torch.rand((M, S), generator=g, dtype=torch.float64) * (t + 1)
        pick = torch.randperm(M * S, generator=g)
        rl.view(-1)[pick[:max(1, M * S // 9)]] = float("nan")
        rl.view(-1)[pick[-max(1, M * S // 7):]] = -0.0
        steps.append(dict(act=torch.randn((M, S), generator=g), logp=torch.randn((M, S), generator=g),
                          feat_c=torch.randn((M, S, 13), generator=g),
                          rew=torch.randn((M, S), generator=g, dtype=torch.float64), rew_light=rl))
    return done, decs, steps


def drive(S, P, E, k, seed):
    """The four specifications over the tape -> (lanes dict, len, cut, current decision, records, done, decs, steps)"""
    from mhppo.external import lanes_begin_torch, lanes_close_torch, lanes_record_torch, lanes_restart_torch
    done, decs, steps = tape(S, P, seed)
    NS = M * S
    recs = (torch.full((T, NS, 13), float("nan")), torch.full((T, NS), float("nan")), torch.full((T, NS), float("nan")),
            torch.full((T, NS), float("nan"), dtype=torch.float64))
    current = types.SimpleNamespace(**{n: getattr(decs[0], n).clone() for n in DEC})
    lanes = lanes_begin_torch(current, E)
    for t in range(k):
        if t >= 1:
            lanes_restart_torch(lanes, t, decs[t], current)
        x = steps[t]
        lanes_record_torch(lanes, t, x["act"], x["logp"], x["feat_c"], x["rew"], x["rew_light"], *recs,
                           torch.from_numpy(done[t]))
    ln, cut = lanes_close_torch(lanes, k)
    return lanes, ln, cut, current, recs, done, decs, steps


@pytest.mark.parametrize("E,k", [(3, T), (3, 4), (1, T), (4, T)])
@pytest.mark.parametrize("S", [1, 3])
def test_bookkeeping_specs_equal_oracle(S, E, k):
    P = 2
    lanes, ln, cut, current, recs, done, decs, steps = drive(S, P, E, k, 10 * S + E)
    want = check_split(done, E, k)
    assert ln.dtype == torch.int32 and cut.dtype == torch.uint8 and lanes["t0"].dtype == torch.int32
    for r in range(M):
        for e in range(E):
            v = e * M + r
            got = (int(lanes["t0"][v]), int(ln[v]), int(cut[v]))
            if e < len(want[r]):
                t0, L, c = want[r][e]
                assert got == (t0, L, c), (r, e)
                for n in DEC:  # the lane's decision is the one drawn from its first row
                    assert eq(lanes[n][v], getattr(decs[t0], n)[r]), (r, e, n)
                for i in range(S):
                    m = 0.0
                    for t in range(t0, t0 + L):
                        m = np_min(m, float(steps[t]["rew_light"][r, i]))
                    assert same_bits(np.float64(m), lanes["ep_min"][v, i].numpy()), (r, e, i)
            else:  # never started
                assert got == (0, 0, 0) and not bool(lanes["exist"][v].any()) and not bool(lanes["a_d"][v].any())
                assert same_bits(lanes["ep_min"][v].numpy(), np.zeros(S))
        t_last = want[r][-1][0]  # the decision in force is the last started lane's
        for n in DEC:
            assert eq(getattr(current, n)[r], getattr(decs[t_last], n)[r]), (r, n)
    # the records: every stream's, idle or not, at wall-clock time
    for t in range(k):
        assert eq(recs[1][t], steps[t]["act"].reshape(-1)) and eq(recs[3][t], steps[t]["rew"].reshape(-1))
        assert eq(recs[0][t], steps[t]["feat_c"].reshape(-1, 13))
    assert bool(torch.isnan(recs[1][k:]).all())
    # close does not change the lanes: an open lane still has len 0
    assert bool(((lanes["len"] == 0) | (cut == 0)).all()) and bool((lanes["len"][cut != 0] == 0).all())


def lanes_batch(S, P, E, k, seed):
    from mhppo.rollout import RolloutBatch
    lanes, ln, cut, current, recs, done, decs, steps = drive(S, P, E, k, seed)
    want, idle = split(done, E, k)
    # a record that belongs to no lane is NaN: none may reach a bucket
    for r in range(M):
        own = np.zeros(T, dtype=bool)
        for t0, L, _ in want[r]:
            own[t0:t0 + L] = True
        for x in recs:
            x[torch.from_numpy(~own), r * S:(r + 1) * S] = float("nan")
    b = RolloutBatch(feat_d=lanes["feat_d"], probs_d=lanes["probs"], logp_d=lanes["logp_d"], a_d=lanes["a_d"],
                     closest=lanes["closest"], exist=lanes["exist"], ep_min=lanes["ep_min"],
                     obs_c_tm=recs[0].reshape(T, M, S, 13), act_tm=recs[1].reshape(T, M, S),
                     logp_tm=recs[2].reshape(T, M, S), rew_tm=recs[3].reshape(T, M, S), rec_of=None, N=M, M=M, S=S, P=P,
                     T=T, lanes=E, t0=lanes["t0"], len=ln, cut=cut, steps=k, feat_tail=None, cut_truncates=True)
    return b, want


def loop_buckets(b, want, fix_bucket, v_boot=None):
    """The lanes buckets by a plain loop in lane-segment order: lane e, stream r, slot i."""
    E, S, P = b.lanes, b.S, b.P
    NS = M * S
    a_d, closest, exist = b.a_d.numpy(), b.closest.numpy(), b.exist.numpy()
    recs = dict(obs=b.obs_c_tm.reshape(T, NS, 13).numpy(), act=b.act_tm.reshape(T, NS).numpy(),
                logp=b.logp_tm.reshape(T, NS).numpy(), rew=b.rew_tm.reshape(T, NS).numpy())
    out = [{k: [] for k in KEYS}, {k: [] for k in KEYS}]
    nseg = [0, 0]
    choice = dict(obs=[], act=[], logp=[], ret=[])
    for e in range(E):
        for r in range(M):
            if e >= len(want[r]):
                assert not exist[e * M + r].any()
                continue
            t0, L, cut = want[r][e]
            v = e * M + r
            for i in range(S):
                if not exist[v, i]:
                    continue
                a = a_d[v, i, closest[v, i]] if fix_bucket else a_d[v].reshape(-1)[i]
                w = 1 if 2 * int(a) - 1 > 0 else 0
                c = r * S + i
                ret = np.zeros(L, dtype=np.float32)
                G = float(np.float64(v_boot[c])) if (cut and v_boot is not None) else 0.0
                for t in range(t0 + L - 1, t0 - 1, -1):
                    G = recs["rew"][t, c] + GAMMA * G
                    ret[t - t0] = np.float32(G)
                for k in ("obs", "act", "logp", "rew"):
                    out[w][k].append(recs[k][t0:t0 + L, c])
                out[w]["ret"].append(ret)
                nseg[w] += 1
                choice["obs"].append(b.feat_d.numpy()[v, i, closest[v, i]])
                choice["act"].append(a_d[v, i, closest[v, i]])
                choice["logp"].append(b.logp_d.numpy()[v, i, closest[v, i]])
                choice["ret"].append(np.float32(b.ep_min.numpy()[v, i]))
    cat = lambda xs, like: np.concatenate(xs) if xs else like[:0, 0]
    return [{k: cat(o[k], recs[k] if k != "ret" else recs["act"]) for k in KEYS} for o in out], nseg, choice


@pytest.mark.parametrize("fix_bucket", [False, True], ids=["rule", "fix_bucket"])
@pytest.mark.parametrize("E,k", [(3, T), (3, 4), (1, T), (4, T)])
@pytest.mark.parametrize("S", [1, 3])
def test_lanes_torch_equals_oracle(S, E, k, fix_bucket):
    from mhppo.rollout import bucket_segments, bucket_segments_lanes_torch
    b, want = lanes_batch(S, 2, E, k, 10 * S + E)
    plan = {}
    cross, wait, choice = bucket_segments_lanes_torch(b, fix_bucket=fix_bucket, plan_out=plan)
    w, nseg, wc = loop_buckets(b, want, fix_bucket)
    assert nseg[0] > 0 and nseg[1] > 0
    for name, got, x, n in (("cross", cross, w[0], nseg[0]), ("wait", wait, w[1], nseg[1])):
        assert got["n_seg"] == n and got["rows"] == x["act"].shape[0], name
        for key in KEYS:
            assert same_bits(got[key].numpy(), x[key]), (name, key)
            assert not bool(torch.isnan(got[key]).any()), (name, key)
    assert set(cross) == set(KEYS) | {"n_seg", "rows"} and set(choice) == {"obs", "act", "logp", "ret", "n_seg", "counts", "rew_sums"}
    assert choice["n_seg"] == nseg[0] + nseg[1] == int(b.exist.sum())
    assert same_bits(choice["obs"].numpy(), np.stack(wc["obs"])) and same_bits(choice["act"].numpy(), np.array(wc["act"], dtype=np.int32))
    assert same_bits(choice["logp"].numpy(), np.array(wc["logp"], dtype=np.float32))
    assert same_bits(choice["ret"].numpy(), np.array(wc["ret"], dtype=np.float32))
    sums = choice["rew_sums"].tolist()
    for i, x in enumerate(w):
        x = x["rew"].astype(np.float32).astype(np.float64)  # two summation orders of n terms
        assert abs(sums[i] - float(x.sum())) <= 2 * (x.size - 1) * 2.0 ** -53 * float(np.abs(x).sum()), i
    x = np.array(wc["ret"], dtype=np.float64)  # a NaN reward_light makes the lane's minimum, and the sum, NaN
    assert np.isnan(x).any() and np.isnan(sums[2])
    # the wait rows start at a multiple of 4; every record in no used lane has ret 0
    row0, pos = plan["row0"], plan["pos"]
    assert bool(((row0 >= 0) == (pos >= 0)).all())
    w0 = (cross["rows"] + 3) // 4 * 4
    assert int(row0[(pos >= 0) & (plan["bucket"] != 0)].min()) == w0 and int(row0[(pos >= 0) & (plan["bucket"] == 0)].min()) == 0
    # bucket_segments dispatches on batch.lanes
    again = bucket_segments(b, fix_bucket=fix_bucket)
    assert again[0]["rows"] == cross["rows"] and eq(again[1]["ret"], wait["ret"]) and eq(again[2]["rew_sums"], choice["rew_sums"])
    with pytest.raises(ValueError):
        bucket_segments(b, gae=(None, None, GAMMA, 0.95))


@pytest.mark.parametrize("S", [1, 3])
def test_cut_bootstrap_starts_only_the_cut_lanes(S):
    from mhppo.rollout import returns_scan_tm_lanes_torch
    E, k = 3, T
    b, want = lanes_batch(S, 2, E, k, 7 + S)
    NS = M * S
    g = torch.Generator().manual_seed(5)
    v_boot = torch.randn(NS, generator=g)
    pos = torch.where(b.exist.reshape(-1) != 0, 0, -1)  # used: the existing lane-segments
    rew = b.rew_tm.reshape(T, NS)
    plain = returns_scan_tm_lanes_torch(rew, M, S, E, GAMMA, pos, b.t0, b.len, b.cut)
    boot = returns_scan_tm_lanes_torch(rew, M, S, E, GAMMA, pos, b.t0, b.len, b.cut, v_boot)
    ex = b.exist.numpy()
    n_cut = n_end = 0
    for r in range(M):
        for e, (t0, L, cut) in enumerate(want[r]):
            for i in range(S):
                c, last = r * S + i, t0 + L - 1
                if not ex[e * M + r, i]:
                    continue
                x = rew[last, c].numpy()
                assert same_bits(plain[last, c].numpy(), np.float32(x))
                if cut:
                    assert same_bits(boot[last, c].numpy(), np.float32(x + GAMMA * np.float64(v_boot[c].numpy())))
                    n_cut += 1
                else:
                    assert same_bits(boot[last, c].numpy(), np.float32(x))
                    assert eq(boot[t0:last + 1, c], plain[t0:last + 1, c])
                    n_end += 1
    assert n_cut > 0 and n_end > 0
    # the whole scan against the loop, and zero outside the used lanes
    w, _, _ = loop_buckets(b, want, False, v_boot.numpy())
    used = torch.zeros((T, NS), dtype=torch.bool)
    for r in range(M):
        for e, (t0, L, cut) in enumerate(want[r]):
            for i in range(S):
                if ex[e * M + r, i]:
                    used[t0:t0 + L, r * S + i] = True
    assert not bool(boot[~used].any()) and not bool(torch.isnan(boot).any())
    assert np.sort(boot[used].numpy()).tobytes() == np.sort(np.concatenate([w[0]["ret"], w[1]["ret"]])).tobytes()


def test_arguments_are_validated():
    from mhppo.external import lanes_begin_torch, lanes_close_torch, lanes_restart_torch
    from mhppo.rollout import bucket_segments_lanes_torch
    b, _ = lanes_batch(1, 2, 3, T, 3)
    for bad in (dict(steps=0), dict(steps=T + 1), dict(len=b.len.long()), dict(t0=b.t0[:5]), dict(cut=b.cut.int()),
                dict(lanes=0)):
        keep = dict(b.__dict__)
        b.__dict__.update(bad)
        with pytest.raises(ValueError):
            bucket_segments_lanes_torch(b)
        b.__dict__.update(keep)
    bucket_segments_lanes_torch(b)
    _, decs, _ = tape(1, 2, 3)
    with pytest.raises(ValueError):
        lanes_begin_torch(decs[0], 0)
    lanes = lanes_begin_torch(decs[0], 2)
    with pytest.raises(ValueError):
        lanes_restart_torch(lanes, 0, decs[1], decs[0])
    with pytest.raises(ValueError):
        lanes_close_torch(lanes, 0)
