"""Worst gap per key between the streaming evaluation statistics (the host harness,
tools/hoststats, through mhppo.stats.stats_from_sums) and get_average on the CPU, over the four
non-choix golden evaluation fixtures and a tiled copy of eval_scalable_221: the figure
tests/evalstats_common.py RTOL is 4x of.  gap = |val - ref| / max(1, |ref|); non-finite entries
must agree exactly and count as 0.

usage: python tools/evalstats_gaps.py [--tile 1024]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hoststats  # noqa: E402
from mhppo.stats import get_average, stats_from_sums  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tile", type=int, default=1024)
a = ap.parse_args()
worst = {}


def run(name, tile=1):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"eval_{name}.npz"))
    v, nc, npd, nl = str(g["variant"]), int(g["nb_car"]), int(g["nb_ped"]), int(g["nb_lines"])
    obs, E, K = g["obs"], len(g["n_obs"]), int(g["episodes"])
    T = obs.shape[0] // (E * K)
    if tile > 1:
        obs, E = np.tile(obs, (tile, 1)), E * tile
    t0 = time.perf_counter()
    ref = get_average(torch.tensor(obs), v, nc, npd, nl)
    t1 = time.perf_counter()
    assert ref["episodes"] == E * K
    got = stats_from_sums(hoststats.stats(obs.reshape(E, K, T, -1).transpose(1, 2, 0, 3), v, nc, npd, nl), nc)
    t2 = time.perf_counter()
    assert set(got) == set(ref)
    for k, r in ref.items():
        x = got[k]
        if not np.isfinite(r):
            assert (np.isnan(r) and np.isnan(x)) or x == r, (k, x, r)
            continue
        worst[k] = max(worst.get(k, 0.0), abs(x - r) / max(1.0, abs(r)))
    print(f"{name} x{tile}: {obs.shape[0]} rows, get_average {t1 - t0:.3f} s, harness + stats_from_sums {t2 - t1:.3f} s")


for n in ("coop_212", "naif_111", "scalable_211", "scalable_221"):
    run(n)
run("scalable_221", a.tile)
for k, v in sorted(worst.items()):
    print(f"{k:32s} {v:.3e}")
print(f"{'worst':32s} {max(worst.values()):.3e}")
