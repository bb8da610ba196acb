"""The minibatch driver's data-parallel orchestration on the CPU with gloo, world size 2
(mhppo.ppo.train_minibatches): the train passes are tests/test_dp_gloo.py's CPU doubles, installed
the way that file installs them and wrapped to record what they are given; every collective is
recorded too.  Each rank shuffles its own shard (the CPU path of mhppo.shuffle.shuffle_batch, the
specification), so the checks are about the orchestration: the same collective sequence on both
ranks, m_global = the sum of the ranks' slice sizes, every local row in exactly one slice per epoch,
and a rank with an empty shard of a head still in every collective."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import shuffle_ref as sr
import test_dp_gloo as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, K = 2, 3
# rows per (head, rank): rank 1 holds no wait rows; the wait head's slice 0 is empty on every rank
# (7 rows, K = 3: bounds 0, 0, 4, 7), so that head sits out step 0 of each epoch
SHARDS = {"cross": (50, 37), "wait": (7, 0), "choice": (30, 21)}
NAMES = ("cross", "wait", "choice")


def _data(name, rank):
    """This rank's shard; obs[:, 0] holds the row's local index (what the doubles' records read)."""
    M = SHARDS[name][rank]
    rng = np.random.default_rng(10 * NAMES.index(name) + rank)
    choice = name == "choice"
    obs = rng.normal(0, 3, (M, 20 if choice else 13)).astype(np.float32)
    obs[:, 0] = np.arange(M)
    act = rng.integers(0, 2, M).astype(np.int32) if choice else rng.normal(-1, 1, M).astype(np.float32)
    return tuple(torch.from_numpy(x) for x in (obs, act, rng.normal(-0.6, 0.3, M).astype(np.float32),
                                               rng.normal(-20, 8, M).astype(np.float32)))


def _run(rank, world, port, per_row, clip, out_q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd")]
    from mhppo import ppo, shuffle
    from mhppo.models import Model_PPO
    G._install_cpu_doubles(ppo)
    log = []
    crit, actr = ppo._critic_pass, ppo._actor_pass

    def critic_pass(p, h, sums, st):
        log.append(("critic", h.kind, p.n_in, p.M, h.m, p.obs[:, 0].tolist(), None))
        crit(p, h, sums, st)

    def actor_pass(p, h, stats, sums, st):
        cn = None if p.counts is None else p.counts.tolist()
        assert (p.act is None) == (h.kind == "d" and not per_row) and (p.counts is None) == (p.act is not None)
        log.append(("actor", h.kind, p.n_in, p.M, h.m, p.obs[:, 0].tolist(), cn))
        actr(p, h, stats, sums, st)

    ppo._critic_pass, ppo._actor_pass = critic_pass, actor_pass
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    real = dist.all_reduce

    def all_reduce(t, *a, **k):
        log.append(("all_reduce", tuple(t.shape), str(t.dtype)))
        return real(t, *a, **k)

    dist.all_reduce = all_reduce
    torch.manual_seed(0)
    nets = [Model_PPO(13, 1, 1, mean=-1.0, std=3.0), Model_PPO(13, 1, 0), Model_PPO(13, 1, 1, mean=-1.0, std=3.0),
            Model_PPO(13, 1, 0), Model_PPO(20, 2, 2), Model_PPO(20, 1, 0)]
    bucket = ppo.GradBucket(nets, "cpu")
    opts = [torch.optim.Adam(n.parameters(), 3e-4 if i % 2 == 0 else 1e-3) for i, n in enumerate(nets)]
    heads = []
    for i, name in enumerate(NAMES):
        obs, act, lp, ret = _data(name, rank)
        m = ppo.global_count(obs.shape[0], "cpu")
        counts = None
        if name == "choice":
            counts = ppo._allreduce_(torch.stack([(act == 0).sum(), (act == 1).sum()]).double())
        heads.append(ppo.Head("d" if name == "choice" else "c", nets[2 * i], nets[2 * i + 1], opts[2 * i],
                              opts[2 * i + 1], obs, act, lp, ret, m, counts, per_row=name == "choice" and per_row))
    del log[:]
    res = ppo.train_minibatches(heads, E, K, lambda e, i: shuffle.shuffle_key(1, 0, e, i, 100 * rank), bucket, clip)
    norms = None
    if clip is not None:
        res, norms = res
        norms = norms.numpy().copy()
    steps = [int(o.state_dict()["state"][0]["step"]) for o in opts]
    weights = [n.flat().detach().numpy().copy() for n in nets]
    out_q.put((rank, log, steps, weights, norms, [None if r is None else r[2] for r in res]))
    dist.destroy_process_group()


def _spawn(per_row, clip):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 32800 + os.getpid() % 1000 + (1 if per_row else 0) + (2 if clip else 0)
    procs = [ctx.Process(target=_run, args=(r, 2, port, per_row, clip, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=240) for _ in range(2)), key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


@pytest.mark.parametrize("per_row,clip", [(False, None), (False, 0.5)])  # (the doubles have no per-row choice loss)
def test_dp2_minibatch_orchestration(per_row, clip):
    (_, log0, steps0, w0, norms0, m0), (_, log1, steps1, w1, norms1, m1) = _spawn(per_row, clip)
    # the same sequence of passes and collectives on both ranks, the rank with no wait rows included
    assert [(x[0], x[1], x[2]) for x in log0] == [(x[0], x[1], x[2]) for x in log1]
    coll = [x for x in log0 if x[0] == "all_reduce"]
    n_counts = 0 if per_row else E
    steps = E * K
    # per call one [H, K] slice-size all-reduce; per epoch one counts all-reduce (none with the per-row
    # loss); per step the advantage sums and the gradient bucket (two runs where the wait head sits out)
    assert coll[0][1] == (3, K)
    assert sum(1 for c in coll if c[1] == (1, K, 2)) == n_counts
    assert sum(1 for c in coll if c[1] == (6,)) == steps
    assert len(coll) == 1 + n_counts + steps + (steps + E)  # E steps reduce the bucket in two runs
    # m_global of every pass is the sum of the ranks' slice sizes; the choice counts are global too
    p0, p1 = ([x for x in lg if x[0] != "all_reduce"] for lg in (log0, log1))
    assert len(p0) == len(p1) == 2 * (3 * steps - E)
    for a, b in zip(p0, p1):
        assert a[4] == b[4] == a[3] + b[3] and a[4] > 0, (a[:5], b[:5])
        assert a[6] == b[6] and (a[6] is None or sum(a[6]) <= a[4])
    # every local row goes through each kind of pass exactly once per epoch
    for rank, passes in enumerate((p0, p1)):
        bc, bw = sr.bounds(SHARDS["cross"][rank], K), sr.bounds(SHARDS["wait"][rank], K)
        for kind in ("critic", "actor"):
            rows = [x[5] for x in passes if x[0] == kind and x[1] == "d"]
            per_epoch = [sum(rows[e * K:(e + 1) * K], []) for e in range(E)]
            for r in per_epoch:
                assert sorted(r) == list(range(SHARDS["choice"][rank]))
            assert per_epoch[0] != per_epoch[1]  # a fresh shuffle per epoch
            # the continuous heads' passes in the driver's order: cross, then wait, per step
            it = iter([x for x in passes if x[0] == kind and x[1] == "c"])
            for e in range(E):
                seen_c, seen_w = [], []
                for j in range(K):
                    x = next(it)
                    assert x[3] == bc[j + 1] - bc[j]
                    seen_c += x[5]
                    if j > 0:  # the wait head sits out step 0 (globally empty slice)
                        y = next(it)
                        assert y[3] == bw[j + 1] - bw[j]
                        seen_w += y[5]
                assert sorted(seen_c) == list(range(SHARDS["cross"][rank]))
                assert sorted(seen_w) == list(range(SHARDS["wait"][rank]))
            assert next(it, None) is None
    # replicated nets and step counts: E K steps, less the steps the wait head sat out
    assert steps0 == steps1 == [steps, steps, steps - E, steps - E, steps, steps]
    for a, b in zip(w0, w1):
        assert np.array_equal(a, b)
    assert m0 == m1 and all(m is not None for m in m0)
    if clip is not None:
        assert norms0.shape == (steps, 6) and np.array_equal(norms0, norms1, equal_nan=True)
        nan = np.isnan(norms0)
        want = np.zeros_like(nan)
        want[0::K, 1] = want[0::K, 4] = True  # the wait head's critic (column 1) and actor (column 3 + 1)
        assert np.array_equal(nan, want)


def _run_algo(rank, world, port, n_total, out_q):
    """Algo_PPO(minibatches=3).train(2) over test_dp_gloo's env and rollout doubles."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd")]
    from mhppo import algo as algo_mod
    from mhppo import ppo
    from mhppo.models import Model_PPO
    G._install_cpu_doubles(ppo)
    algo_mod.Env_rollout = G._rollout_double_class(n_total)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    log = []
    real = dist.all_reduce

    def all_reduce(t, *a, **k):
        log.append(tuple(t.shape))
        return real(t, *a, **k)

    dist.all_reduce = all_reduce
    n = n_total // world
    torch.manual_seed(0)
    # verbose on rank 0 (it prints the reference's progress lines): last_losses is formed there
    a = algo_mod.Algo_PPO(Model_PPO, G._VenvDouble(n, rank * n), verbose=rank == 0, save_curves=False,
                          num_states_d=20, minibatches=3)
    a.train(2)
    steps = [int(o.state_dict()["state"][0]["step"]) for o in a._optimizers().values()]
    out_q.put((rank, log, steps, [net.flat().detach().numpy().copy() for net in a.nets()], a.last_losses))
    dist.destroy_process_group()


def test_dp4_algo_minibatches():
    """Whole iterations under data parallelism (rank 1 holds no wait rows, rank 2 no cross rows):
    update()'s one counts all-reduce carries the [3, K] slice sizes, every rank issues the same
    collectives, the nets stay replicated and every optimiser takes 10 K steps per iteration."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33900 + os.getpid() % 1000
    procs = [ctx.Process(target=_run_algo, args=(r, 4, port, 64, q)) for r in range(4)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=300) for _ in range(4)), key=lambda x: x[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    logs = [g[1] for g in got]
    assert all(lg == logs[0] for lg in logs)
    assert logs[0][0] == (3 + 3 * 3 + 2,) and (3, 3) not in logs[0]  # rows, slice sizes, counts: one all-reduce
    assert all(g[2] == [60] * 6 for g in got)
    losses = got[0][4]  # per head (actor, critic) mean losses of its last minibatch step
    assert sorted(losses) == ["choice", "cross", "wait"]
    assert all(np.isfinite(v).all() and v[1] > 0 for v in losses.values())
    for g in got[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got[0][3], g[3]))


def test_constructor_refuses_on_cpu():
    from mhppo.algo import Algo_PPO
    from mhppo.models import Model_PPO
    for bad in (0, -3, True, False, 1.5, "2"):
        with pytest.raises(ValueError, match="minibatches"):
            Algo_PPO(Model_PPO, None, minibatches=bad)
