"""ctypes wrapper of tools/libhostpolicy.so: the stateless policy (mhppo_policy_dims / _decide /
_act) compiled for the CPU from the device source (csrc/policy_rule.h).  numpy in, numpy out."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
L = ctypes.CDLL(os.path.join(HERE, "libhostpolicy.so"))
P, F, I64 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int64
VARIANTS = {"coop": 0, "4cars": 1, "scalable": 2, "naif": 3, "4cars2": 4, "stop": 5}
CAR_B = ((-4.0, 10.0), (2.0, 10.0))


class EnvCfg(ctypes.Structure):  # mhppo_env_cfg (include/mhppo.h)
    _fields_ = [("variant", ctypes.c_int32), ("n_envs", ctypes.c_int32), ("nb_car", ctypes.c_int32),
                ("nb_ped", ctypes.c_int32), ("nb_lines", ctypes.c_int32), ("max_episode", ctypes.c_int32),
                ("sin_model", ctypes.c_int32), ("flags", ctypes.c_int32), ("dt", ctypes.c_double),
                ("car_b", ctypes.c_double * 4), ("ped_b", ctypes.c_double * 8), ("cross_b", ctypes.c_double * 2),
                ("seed_base", ctypes.c_uint64), ("env_id_offset", ctypes.c_uint64)]


for _name, _args in (("hp_dims", [ctypes.POINTER(EnvCfg), P]),
                     ("hp_decide", [ctypes.POINTER(EnvCfg), P, P, I64, P, P]),
                     ("hp_act", [ctypes.POINTER(EnvCfg), P, F, F, P, F, F, P, P, I64, P]),
                     ("hp_features", [ctypes.POINTER(EnvCfg), P, I64, P]),
                     ("hp_features_d", [ctypes.POINTER(EnvCfg), P, I64, P])):
    getattr(L, _name).restype = ctypes.c_int
    getattr(L, _name).argtypes = _args


def cfg(variant, nb_car, nb_ped, nb_lines, dt=0.3, car_b=CAR_B):
    """The part of an mhppo_env_cfg the policy reads (the rest stays zero)."""
    c = EnvCfg()
    c.variant = VARIANTS[variant] if isinstance(variant, str) else int(variant)
    c.n_envs, c.nb_car, c.nb_ped, c.nb_lines, c.max_episode, c.dt = 1, nb_car, nb_ped, nb_lines, 80, dt
    for i, v in enumerate(np.asarray(car_b, np.float64).reshape(-1)):
        c.car_b[i] = v
    return c


def _p(a):
    return None if a is None else a.ctypes.data_as(P)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def dims(c):
    """(obs_dim, S, P, choice_dim)"""
    out = np.zeros(4, np.int32)
    if L.hp_dims(ctypes.byref(c), _p(out)) != 0:
        raise ValueError("hp_dims: the config is refused")
    return tuple(int(x) for x in out)


def _obs(c, obs):
    od, S, Pn, dc = dims(c)
    obs = _f32(obs)
    if obs.ndim != 2 or obs.shape[1] != od:
        raise ValueError(f"obs must be [M, {od}], got {obs.shape}")
    return obs, S, Pn, dc


def decide(c, w_choice, obs, probs=False):
    """a_d int32 [M, S, P] (and probs float32 [M, S, P, 2])"""
    obs, S, Pn, dc = _obs(c, obs)
    w = _f32(w_choice)
    if w.size != 32 * dc + 4224 + 66:
        raise ValueError(f"the choice actor of this config has {dc} inputs")
    M = obs.shape[0]
    a_d = np.zeros((M, S, Pn), np.int32)
    pr = np.zeros((M, S, Pn, 2), np.float32) if probs else None
    if L.hp_decide(ctypes.byref(c), _p(w), _p(obs), M, _p(a_d), _p(pr)) != 0:
        raise ValueError("hp_decide: the config is refused")
    return (a_d, pr) if probs else a_d


def act(c, w_cross, w_wait, obs, a_d, mean=-1.0, std=3.0):
    """actions float64 [M, 2 S] = [acc.., light..]"""
    obs, S, Pn, dc = _obs(c, obs)
    wc, ww = _f32(w_cross), _f32(w_wait)
    if wc.size != 32 * 13 + 4224 + 33 or ww.size != wc.size:
        raise ValueError("the continuous actors are 13 -> 1")
    M = obs.shape[0]
    a_d = np.ascontiguousarray(a_d, np.int32)
    if a_d.shape != (M, S, Pn):
        raise ValueError(f"a_d must be [{M}, {S}, {Pn}], got {a_d.shape}")
    out = np.zeros((M, 2 * S), np.float64)
    if L.hp_act(ctypes.byref(c), _p(wc), float(mean), float(std), _p(ww), float(mean), float(std), _p(obs), _p(a_d), M,
                _p(out)) != 0:
        raise ValueError("hp_act: the config is refused")
    return out


def features_d(c, obs):
    """The obs_car_ped_d choice features of every triple: float32 [M, S, P, choice_dim]"""
    obs, S, Pn, dc = _obs(c, obs)
    out = np.zeros((obs.shape[0], S, Pn, dc), np.float32)
    if L.hp_features_d(ctypes.byref(c), _p(obs), obs.shape[0], _p(out)) != 0:
        raise ValueError("hp_features_d: the config is refused")
    return out


def features(c, obs):
    """The 13 obs_car_ped features of every triple: float32 [M, S, P, 13]"""
    obs, S, Pn, dc = _obs(c, obs)
    out = np.zeros((obs.shape[0], S, Pn, 13), np.float32)
    if L.hp_features(ctypes.byref(c), _p(obs), obs.shape[0], _p(out)) != 0:
        raise ValueError("hp_features: the config is refused")
    return out
