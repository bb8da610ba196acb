"""Cost of the opt-in minibatch update (Algo_PPO(minibatches=K), mhppo.ppo.train_minibatches) and
of its shuffle (mhppo_batch_shuffle, csrc/batch_shuffle.hip).

Shuffle alone: HIP events around single launches after warm-up, medians, at 10 485 760 x 13 (a
continuous head of config 3) and 262 144 x 27 (its choice head, with the per-slice counts launch);
bytes moved = 2 * M * (n_in + 3) * 4 (every row read once and written once) over the time.  Beside
it the same head's two train passes of one epoch (ppo.train_epoch on one head, less its Adam step:
events around the critic and the actor launch), from the same process.

--algo: wall clock around synchronised Algo_PPO.train(1) iterations at config 2 (coop 2/1/2, 4096
envs) and config 3 (4cars 4/1/2, 65536 envs), the default path and minibatches=K alternating,
medians.

usage: python tools/bench_minibatch.py [--reps R] [--K K] [--algo] [--iters I]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd")]
import torch  # noqa: E402

CONFIGS = {2: ("coop", 2, 1, 2, 4096), 3: ("4cars", 4, 1, 2, 65536)}

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--K", type=int, default=8)
ap.add_argument("--algo", action="store_true")
ap.add_argument("--iters", type=int, default=8)
a = ap.parse_args()

from mhppo import ppo, shuffle  # noqa: E402
from mhppo.models import Model_PPO  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


for M, n_in, choice in ((10_485_760, 13, False), (262_144, 27, True)):
    g = torch.Generator(device=DEV).manual_seed(0)
    obs = torch.randn(M, n_in, device=DEV, generator=g)
    act = (torch.rand(M, device=DEV, generator=g) < 0.4).to(torch.int32) if choice else torch.randn(M, device=DEV, generator=g)
    logp, ret = -torch.rand(M, device=DEV, generator=g), torch.randn(M, device=DEV, generator=g)
    src = (obs, act, logp, ret)
    dst = tuple(torch.empty_like(t) for t in src)
    counts = torch.zeros(a.K, 2, dtype=torch.float64, device=DEV) if choice else None
    keys = iter(range(1, 10**6))
    med, lo, hi = timed(lambda: shuffle.shuffle_batch(src, dst, next(keys), a.K, counts), a.reps)
    nbytes = 2 * M * (n_in + 3) * 4
    print(f"shuffle {M} x {n_in}{' + counts' if choice else ''}: {med * 1e3:8.1f} us (min {lo * 1e3:.1f} max {hi * 1e3:.1f})"
          f"   {nbytes / 1e6:.1f} MB moved, {nbytes / med / 1e9:.2f} TB/s", flush=True)
    # the same head's two train passes of one epoch (full batch), launch by launch
    torch.manual_seed(0)
    actor = Model_PPO(n_in, 2 if choice else 1, 2 if choice else 1, mean=-1.0, std=3.0).to(DEV)
    critic = Model_PPO(n_in, 1, 0).to(DEV)
    cn = torch.stack([(act == 0).sum(), (act == 1).sum()]).double() if choice else None
    head = ppo.Head("d" if choice else "c", actor, critic, None, None, obs, act, logp, ret, M, cn)
    plan = ppo._HeadPlan(head)
    sums = torch.zeros(2, 3, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    c_med, _, _ = timed(lambda: ppo._critic_pass(plan, head, sums[0], st), a.reps)
    a_med, _, _ = timed(lambda: ppo._actor_pass(plan, head, sums[0, 1:3], sums[1], st), a.reps)
    print(f"  train passes of one epoch on the same rows: critic {c_med * 1e3:.1f} us + actor {a_med * 1e3:.1f} us = "
          f"{(c_med + a_med) * 1e3:.1f} us; the shuffle is {med / (c_med + a_med):.2f} of them", flush=True)
    del obs, act, logp, ret, src, dst, plan, head
    torch.cuda.empty_cache()

if a.algo:
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk

    def make_algo(cfg, **kw):
        variant, nc, npd, nl, n = CONFIGS[cfg]
        venv = VecCrosswalk(variant, n, nc, npd, nl, seed_base=0)
        torch.manual_seed(0)
        return Algo_PPO(Model_PPO, venv, verbose=False, save_curves=False, **kw)

    for cfg in (2, 3):
        algos = {}
        for on in (False, True):
            algos[on] = make_algo(cfg, minibatches=a.K if on else None)
            algos[on].train(2)  # warm-up (allocator, Adam state, plans)
            torch.cuda.synchronize()
        ms = {False: [], True: []}
        for _ in range(a.iters):
            for on in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                algos[on].train(1)
                torch.cuda.synchronize()
                ms[on].append((time.perf_counter() - t0) * 1e3)
        off_ms, on_ms = statistics.median(ms[False]), statistics.median(ms[True])
        print(f"config {cfg}: Algo_PPO.train(1) full-batch {off_ms:.2f} ms, minibatches={a.K} {on_ms:.2f} ms "
              f"({on_ms - off_ms:+.2f} ms per iteration)   off {[round(x, 2) for x in ms[False]]} "
              f"on {[round(x, 2) for x in ms[True]]}", flush=True)
        del algos
        torch.cuda.empty_cache()
