"""Shared by tests/test_evalstats_host.py and tests/test_evalstats_gpu.py: the reference's golden
evaluation trajectories as [K, T, E, obs_dim] rows, and the comparison of a streaming-statistics
dict with get_average's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

FIXTURES = ("coop_212", "naif_111", "scalable_211", "scalable_221")  # the non-choix eval_*.npz
EXACT = ("episodes", "yield_share", "go_share", "could_stop_share", "scenario_yield_yield", "scenario_go_go",
         "scenario_go_yield", "scenario_yield_go")
F64 = ("mean_waiting_time", "std_waiting_time")  # float64 on both sides
RTOL_F64 = 1e-9
# The other entries are float32 torch reductions in get_average against float64 sums here.  Worst
# gap |val - ref| / max(1, |ref|) between the host harness and get_average, measured on the CPU
# over the four fixtures and a 1 024-fold tiled eval_scalable_221 (655 360 rows): 1.922e-07
# (mean_speed_car0; per key in DESIGN.md).  The bound is 4x that: the gap is the float32
# reduction's rounding, not an error of the streaming path.
RTOL = 4 * 1.922e-07


def load_fixture(name):
    """(traj [K, T, E, od] float32, obs [E*K*T, od] env-major as get_average takes it, variant,
    nb_car, nb_ped, nb_lines, E, K, T)."""
    g = np.load(os.path.join(GOLDEN, f"eval_{name}.npz"))
    obs = g["obs"]
    E, K = len(g["n_obs"]), int(g["episodes"])
    T = obs.shape[0] // (E * K)
    assert E * K * T == obs.shape[0] and (E, K, T) == (4, 2, 80)
    traj = np.ascontiguousarray(obs.reshape(E, K, T, -1).transpose(1, 2, 0, 3))
    return dict(traj=traj, obs=obs, variant=str(g["variant"]), nb_car=int(g["nb_car"]), nb_ped=int(g["nb_ped"]),
                nb_lines=int(g["nb_lines"]), E=E, K=K, T=T, seed_base=int(g["seed_base"]))


def check_dict(got, ref, keys=None):
    """got (stats_from_sums) against ref (get_average's dict, or a golden's entries)."""
    keys = list(ref) if keys is None else keys
    for k in keys:
        r, v = float(ref[k]), float(got[k])
        print(f"{k:32s} got {v!r:26} ref {r!r:26}")
        if np.isnan(r):
            assert np.isnan(v), (k, v, r)
        elif np.isinf(r):
            assert v == r, (k, v, r)
        elif k in EXACT:
            assert v == r, (k, v, r)
        else:
            rtol = RTOL_F64 if k in F64 else RTOL
            assert abs(v - r) <= rtol * max(1.0, abs(r)), (k, v, r, abs(v - r) / max(1.0, abs(r)))
