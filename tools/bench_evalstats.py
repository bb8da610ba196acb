"""Streaming evaluation statistics (Algo_PPO.evaluate_stats) against the trajectory path
(Algo_PPO.evaluate followed by get_average) at one shape: wall clock around synchronised calls,
alternating, medians; the baseline split into its loop and get_average; and the row kernel alone
(mhppo_eval_stats_row): HIP events around single launches, with the bytes it moves (the row read,
the carry read and written, the row-level accumulators read and written) against the HBM peak.

usage: python tools/bench_evalstats.py [--variant coop --cars 2 --peds 1 --lines 2] [--envs N]
                                       [--episodes K] [--reps R] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd")]
import torch  # noqa: E402

from mhppo.algo import Algo_PPO  # noqa: E402
from mhppo.env import VecCrosswalk  # noqa: E402
from mhppo.models import Model_PPO  # noqa: E402
from mhppo.rollout import EvalStats  # noqa: E402
from mhppo.stats import EVS_N  # noqa: E402

HBM_PEAK = 8.0e12  # MI355X, bytes / s

ap = argparse.ArgumentParser()
ap.add_argument("--variant", default="coop")
ap.add_argument("--cars", type=int, default=2)
ap.add_argument("--peds", type=int, default=1)
ap.add_argument("--lines", type=int, default=2)
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--episodes", type=int, default=2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--row-reps", type=int, default=100)
ap.add_argument("--json", default="")
a = ap.parse_args()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


torch.manual_seed(0)
venv = VecCrosswalk(a.variant, a.envs, a.cars, a.peds, a.lines, seed_base=0)
algo = Algo_PPO(Model_PPO, venv, verbose=False)
K = a.episodes
res = {"variant": a.variant, "cars": a.cars, "peds": a.peds, "lines": a.lines, "envs": a.envs, "episodes": K,
       "obs_dim": venv.obs_dim, "reps": a.reps}
# warm-up of both paths (allocator, module load)
algo.get_average(algo.evaluate(1)[0])
algo.evaluate_stats(1)
ms = {"evaluate": [], "get_average": [], "evaluate_stats": []}
peak = {}
for _ in range(a.reps):
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t_loop, out = wall(lambda: algo.evaluate(K))
    t_avg, ref = wall(lambda: algo.get_average(out[0]))
    peak["evaluate+get_average"] = torch.cuda.max_memory_allocated() - base
    del out
    ms["evaluate"].append(t_loop)
    ms["get_average"].append(t_avg)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t_new, got = wall(lambda: algo.evaluate_stats(K))
    peak["evaluate_stats"] = torch.cuda.max_memory_allocated() - base
    ms["evaluate_stats"].append(t_new)
med = {k: statistics.median(v) for k, v in ms.items()}
res.update(ms=ms, ms_median=med, peak_bytes=peak, episodes_ref=ref["episodes"], episodes_stats=got["episodes"])
print(f"{a.variant} {a.cars}/{a.peds}/{a.lines}, {a.envs} envs, K = {K}, obs_dim {venv.obs_dim}")
print(f"  evaluate(K)            {med['evaluate']:10.1f} ms   (min {min(ms['evaluate']):.1f} max {max(ms['evaluate']):.1f})")
print(f"  get_average            {med['get_average']:10.1f} ms   (min {min(ms['get_average']):.1f} max {max(ms['get_average']):.1f})")
print(f"  baseline total         {med['evaluate'] + med['get_average']:10.1f} ms   peak {peak['evaluate+get_average'] / 1e6:.1f} MB")
print(f"  evaluate_stats(K)      {med['evaluate_stats']:10.1f} ms   (min {min(ms['evaluate_stats']):.1f} "
      f"max {max(ms['evaluate_stats']):.1f})   peak {peak['evaluate_stats'] / 1e6:.1f} MB", flush=True)

# ---- the row kernel alone, on the env's current observation (rows 1 .. T-2: no episode closes)
acc = EvalStats(venv)
acc.begin()
obs = venv.reset()
T = venv.max_episode
acc.row(obs, 0, T)
for _ in range(5):
    acc.row(obs, 1, T)
torch.cuda.synchronize()
each = []
for _ in range(a.row_reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    acc.row(obs, 1, T)
    e1.record()
    e1.synchronize()
    each.append(e0.elapsed_time(e1) * 1e3)
S, P, nc = venv.n_slots, venv.nb_ped, venv.nb_car
carry = 4 * (1 + 2 * P + 5 * nc) + 4 * (2 * P + nc)
moved = a.envs * (4 * venv.obs_dim + 2 * carry + 2 * 8 * 8)  # row read + carry r/w + 8 row-level accumulators r/w
us = statistics.median(each)
res["row_kernel"] = {"us_median": us, "us_min": min(each), "us_max": max(each), "bytes": moved,
                     "row_bytes": a.envs * 4 * venv.obs_dim, "gb_per_s": moved / us / 1e3,
                     "frac_hbm_peak": moved / (us * 1e-6) / HBM_PEAK, "state_bytes": acc.state.numel() * 8,
                     "sums": EVS_N}
print(f"  row kernel             {us:10.1f} us   (min {min(each):.1f} max {max(each):.1f})  {moved / 1e6:.2f} MB moved, "
      f"{moved / us / 1e3:.0f} GB/s = {100 * res['row_kernel']['frac_hbm_peak']:.1f} % of the HBM peak")
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
