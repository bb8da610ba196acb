"""Time of the ragged bucketing (batches with early episode ends, mhppo.rollout.bucket_segments_ragged_native)
against the fixed-length bucketing on the same rollout batch: config 3's shape by default (4cars, 65 536 envs x
4 slots, T = 80).  Three variants of one collected batch, alternating within every repetition:
  fixed    bucket_segments on the batch as collected
  never    the same batch with len = 0 everywhere (no stream ended): the ragged path on the same rows
  sched    stream r ends after 1 + (7 r) mod T steps, every fifth never: about half the rows
Each call is timed by the host clock between two device synchronisations (the bucketing has one host read
of its own inside).  Prints the median, minimum and maximum in ms over --reps repetitions.

    python tools/bench_early_end.py [--envs 65536] [--reps 20]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mh-ppo_amd"))


def main():
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    from mhppo.rollout import RolloutBatch, RolloutGPU, bucket_segments
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    N = a.envs
    venv = VecCrosswalk("4cars", N, 4, 1, 2, seed_base=0)
    ro = RolloutGPU(venv)
    T = ro.T
    torch.manual_seed(0)
    ac, aw = (Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda() for _ in range(2))
    ad = Model_PPO(ro.dc, 2, 2).cuda()
    batch = ro.collect(ac, aw, ad, seed=0, iteration=0)
    r = torch.arange(N, device="cuda")
    lens = torch.where(r % 5 == 4, torch.zeros_like(r), 1 + (7 * r) % T).to(torch.int32)
    variants = {"fixed": batch,
                "never": RolloutBatch(**batch.__dict__, len=torch.zeros(N, dtype=torch.int32, device="cuda"), steps=T),
                "sched": RolloutBatch(**batch.__dict__, len=lens, steps=T)}

    def timed(b):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = bucket_segments(b)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    rows = {}
    for name, b in variants.items():  # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            _, out = timed(b)
        rows[name] = out[0]["ret"].numel() + out[1]["ret"].numel()
    ms = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, b in variants.items():
            ms[name].append(timed(b)[0])
    print(f"4cars, {N} envs x {ro.S} slots, T = {T}, {a.reps} repetitions, alternating")
    for name, v in ms.items():
        print(f"  {name:6s} {rows[name]:10d} rows  median {statistics.median(v):8.3f} ms  (min {min(v):.3f}, max {max(v):.3f})")


if __name__ == "__main__":
    main()
