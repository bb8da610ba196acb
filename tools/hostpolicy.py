"""ctypes wrapper of tools/libhostpolicy.so: the stateless policy (mhppo_policy_dims / _decide /
_act, and the stochastic rule of mhppo_policy_sample_decide / _sample_act) compiled for the CPU from the
device source (csrc/policy_rule.h, csrc/policy_sample_rule.h).  numpy in, numpy out."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
L = ctypes.CDLL(os.path.join(HERE, "libhostpolicy.so"))
P, F, I64, U64 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int64, ctypes.c_uint64
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
                     ("hp_features_d", [ctypes.POINTER(EnvCfg), P, I64, P]),
                     ("hp_sample_decide", [ctypes.POINTER(EnvCfg), P, P, I64, P, P, U64, U64] + [P] * 7),
                     ("hp_sample_act", [ctypes.POINTER(EnvCfg), P, F, F, P, F, F, P, P, P, I64, P, U64, U64, I64]
                      + [P] * 5),
                     ("hp_sample_noise", [ctypes.POINTER(EnvCfg), I64, U64, U64, I64, P, P])):
    getattr(L, _name).restype = ctypes.c_int
    getattr(L, _name).argtypes = _args
L.hp_set_threads.restype = ctypes.c_int
L.hp_set_threads.argtypes = [ctypes.c_int]


def set_threads(n):
    """Threads of decide / act / sample_decide / sample_act's row loops from here on: 1 .. 16 (1: the plain
    loop), 0: one per CPU, 16 at most (the default).  Returns the previous setting."""
    return int(L.hp_set_threads(int(n)))


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


MASK64 = (1 << 64) - 1


def noise_key(seed, iteration):
    """The collector's Philox key (RolloutGPU.draw_noise)."""
    return (int(seed) * 1000003 + int(iteration)) & MASK64


def _one_noise(*sources):
    if sum(x is not None for x in sources) != 1:
        raise ValueError("exactly one noise source: a tape, forced decisions or a Philox key")


def sample_decide(c, w_choice, obs, u=None, forced=None, key=None, first_env=0, features=True):
    """The stochastic decide over rows: dict of a_d int32, logp_d [M, S, P], probs [M, S, P, 2],
    feat_d [M, S, P, choice_dim] (features=True), closest int32, exist uint8 [M, S] and status (int)."""
    _one_noise(u, forced, key)
    obs, S, Pn, dc = _obs(c, obs)
    w = _f32(w_choice)
    if w.size != 32 * dc + 4224 + 66:
        raise ValueError(f"the choice actor of this config has {dc} inputs")
    M = obs.shape[0]
    if u is not None:
        u = _f32(u)
        assert u.shape == (M, S, Pn)
    if forced is not None:
        forced = np.ascontiguousarray(forced, np.int32)
        assert forced.shape == (M, S, Pn)
    out = dict(a_d=np.zeros((M, S, Pn), np.int32), logp_d=np.zeros((M, S, Pn), np.float32),
               probs=np.zeros((M, S, Pn, 2), np.float32), feat_d=np.zeros((M, S, Pn, dc), np.float32) if features else None,
               closest=np.zeros((M, S), np.int32), exist=np.zeros((M, S), np.uint8))
    st = np.zeros(1, np.uint32)
    if L.hp_sample_decide(ctypes.byref(c), _p(w), _p(obs), M, _p(u), _p(forced), int(key or 0) & MASK64,
                          int(first_env) & MASK64, _p(out["a_d"]), _p(out["logp_d"]), _p(out["probs"]),
                          _p(out["feat_d"]), _p(out["closest"]), _p(out["exist"]), _p(st)) != 0:
        raise ValueError("hp_sample_decide: refused")
    out["status"] = int(st[0])
    return out


def sample_act(c, w_cross, w_wait, obs, a_d, closest, eps=None, key=None, first_env=0, t=0, mean=-1.0, std=3.0,
               mean_wait=None, std_wait=None):
    """The stochastic act over rows: dict of actions float64 [M, 2 S], act, logp float32 [M, S],
    feat_c [M, S, 13] and status (int)."""
    _one_noise(eps, key)
    obs, S, Pn, dc = _obs(c, obs)
    wc, ww = _f32(w_cross), _f32(w_wait)
    if wc.size != 32 * 13 + 4224 + 33 or ww.size != wc.size:
        raise ValueError("the continuous actors are 13 -> 1")
    M = obs.shape[0]
    a_d = np.ascontiguousarray(a_d, np.int32)
    closest = np.ascontiguousarray(closest, np.int32)
    if a_d.shape != (M, S, Pn) or closest.shape != (M, S):
        raise ValueError(f"a_d must be [{M}, {S}, {Pn}] and closest [{M}, {S}]")
    if eps is not None:
        eps = _f32(eps)
        assert eps.shape == (M, S)
    mw = mean if mean_wait is None else mean_wait
    sw = std if std_wait is None else std_wait
    out = dict(actions=np.zeros((M, 2 * S), np.float64), act=np.zeros((M, S), np.float32),
               logp=np.zeros((M, S), np.float32), feat_c=np.zeros((M, S, 13), np.float32))
    st = np.zeros(1, np.uint32)
    if L.hp_sample_act(ctypes.byref(c), _p(wc), float(mean), float(std), _p(ww), float(mw), float(sw), _p(obs), _p(a_d),
                       _p(closest), M, _p(eps), int(key or 0) & MASK64, int(first_env) & MASK64, int(t),
                       _p(out["actions"]), _p(out["act"]), _p(out["logp"]), _p(out["feat_c"]), _p(st)) != 0:
        raise ValueError("hp_sample_act: refused")
    out["status"] = int(st[0])
    return out


def sample_noise(c, M, key, first_env=0, t=0):
    """The in-rule Philox noise of rows [0, M): (u float32 [M, S, P], eps float32 [M, S] of step t)."""
    od, S, Pn, dc = dims(c)
    u, eps = np.zeros((M, S, Pn), np.float32), np.zeros((M, S), np.float32)
    if L.hp_sample_noise(ctypes.byref(c), M, int(key) & MASK64, int(first_env) & MASK64, int(t), _p(u), _p(eps)) != 0:
        raise ValueError("hp_sample_noise: refused")
    return u, eps
