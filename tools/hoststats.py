"""ctypes wrapper of tools/libhoststats.so: the streaming evaluation statistics compiled for the
CPU from the device source (csrc/eval_stats_terms.h).  numpy in, numpy out."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
L = ctypes.CDLL(os.path.join(HERE, "libhoststats.so"))
P = ctypes.c_void_p
L.hs_n.restype = ctypes.c_int
L.hs_stats.restype = ctypes.c_int
L.hs_stats.argtypes = [ctypes.c_int] * 5 + [P] + [ctypes.c_int64] * 3 + [P, P]
EVS_N = L.hs_n()
VARIANT = {"coop": 0, "4cars": 1, "scalable": 2, "naif": 3, "4cars2": 4, "stop": 5}  # include/mhppo.h MHPPO_*


def stats(traj, variant, nb_car, nb_ped, nb_lines, want_abs=False):
    """traj float32 [K, T, E, obs_dim] (episode, row, env) -> the MHPPO_EVS_N float64 sums
    (want_abs: also the sums of |term|).  ValueError for T < 2 or a layout get_average rejects."""
    traj = np.ascontiguousarray(traj, np.float32)
    K, T, E, od = traj.shape
    slots = 2 * nb_lines if variant == "scalable" else nb_car
    sums, abs_sums = np.zeros(EVS_N), np.zeros(EVS_N)
    rc = L.hs_stats(VARIANT[variant], slots, nb_car, nb_ped, od, traj.ctypes.data_as(P), K, T, E,
                    sums.ctypes.data_as(P), abs_sums.ctypes.data_as(P))
    if rc != 0:
        raise ValueError(f"hs_stats: T = {T} / variant {variant!r} ({nb_car} cars, {nb_ped} peds, width {od}) "
                         f"not supported")
    return (sums, abs_sums) if want_abs else sums
