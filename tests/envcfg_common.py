"""Non-default env configurations shared by tests/test_env_config.py (CPU) and
tests/test_env_config_gpu.py: the four configurations of tests/golden/gen/make_env_golden.py
CONFIGS, the envcfg_*.npz fixtures recorded from the reference at them, and the forced action
stream of the many-env comparisons.

B2 are bounds whose -2 * car_b[0][0] = 6 is no power of two, so the env's braking distance
v^2 / (-2 b00) takes its true division instead of the power-of-two reciprocal (env_body.h
build_cfg, brake_p2).
"""
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B2 = dict(car_b=((-3.0, 8.0), (1.5, 8.0)), ped_b=((-0.1, 0.5, 0.0, -4.0), (0.1, 2.0, 3.0, -0.25)),
          cross_b=(3.0, 3.5))
DEFAULT = dict(dt=0.3, max_episode=80, simulation="sin")
CONFIGS = {
    "A": dict(dt=0.3, max_episode=80, simulation="unif"),
    "B": dict(dt=0.2, max_episode=50, simulation="sin"),
    "C": dict(dt=0.3, max_episode=80, simulation="sin", **B2),
    "D": dict(dt=0.5, max_episode=25, simulation="unif", **B2),
}
SHAPES = [("coop", 2, 1, 2), ("coop", 4, 3, 2), ("4cars", 4, 1, 2), ("scalable", 8, 1, 4), ("scalable", 4, 3, 2),
          ("naif", 1, 1, 1), ("stop", 2, 2, 2)]
FILES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "envcfg_*.npz")))
FILE_IDS = [os.path.basename(f)[7:-4] for f in FILES]


def shape_id(s):
    return f"{s[0]}_{s[1]}{s[2]}{s[3]}"


def fixture_cfg(g):
    """The configuration an envcfg_*.npz fixture was recorded at, as VecCrosswalk / HostVec keywords."""
    return dict(dt=float(g["dt"]), max_episode=int(g["max_episode"]), simulation=str(g["simulation"]),
                car_b=g["car_b"], ped_b=g["ped_b"], cross_b=g["cross_b"])


def acc_bounds(cfg):
    cb = cfg.get("car_b", ((-4.0, 10.0), (2.0, 10.0)))
    return float(cb[0][0]), float(cb[1][0])


def action_stream(cfg, n, slots, steps, seed=1):
    """float64 [steps, n, 2 * slots]: accelerations uniform in [acc_min - 0.5, acc_max + 0.5] rounded through
    float32 (what a float32 policy hands the env), one fixed light in {-1, +1} per env and slot."""
    rng = np.random.default_rng(seed)
    lo, hi = acc_bounds(cfg)
    light = rng.choice([-1.0, 1.0], size=(n, slots))
    acc = rng.uniform(lo - 0.5, hi + 0.5, size=(steps, n, slots)).astype(np.float32).astype(np.float64)
    return np.concatenate([acc, np.broadcast_to(light, acc.shape)], 2)


# ---- the stateless policy's rule at a non-default dt / car_b ------------------------------------
# dt 0.2 and 0.5 on the B2 car bounds (a -3 / +1.5 clamp instead of -4 / +2)
POLICY_CFGS = {"dt02": dict(dt=0.2, max_episode=50, simulation="sin", **B2), "dt05": CONFIGS["D"]}


def speed_rows(obs, n_slots, cfg, seed=3):
    """A copy of the observation rows obs [M, od] in which every second row's car speeds (column 1 of each
    slot's block) are redrawn so that (10 - V) / dt is uniform in [b00 - 1, b10 + 1]: speeds near the
    limit of 10, on both sides of both clamps of the left-lane override."""
    rng = np.random.default_rng(seed)
    b00, b10 = acc_bounds(cfg)
    out = np.array(obs, np.float32)
    cw = 7 if out.shape[1] - 7 * n_slots - 4 >= 0 and (out.shape[1] - 7 * n_slots - 4) % 9 == 0 else 6
    x = rng.uniform(b00 - 1.0, b10 + 1.0, (len(out[::2]), n_slots))
    out[::2, 1:cw * n_slots:cw] = (10.0 - x * cfg["dt"]).astype(np.float32)
    return out


def policy_act_ref(f, a_d, head_cross, head_wait, cfg):
    """The deterministic rule in plain float64 (Env_rollout.iterations :193-207): f float32 [M, S, P, 13]
    the (slot, pedestrian) features, a_d [M, S, P] the choices, head_* float32 [M, S, P] the two actors'
    outputs on f.  Returns (actions float64 [M, 2 S], regimes) with regimes a dict of boolean [M, S, P]
    masks: where the override clamps at b00, at b10, lies strictly between, and where the cap binds."""
    b00, b10 = acc_bounds(cfg)
    M, S, P = a_d.shape
    cap = (10.0 - f[..., 0].astype(np.float64)) / cfg["dt"]
    ovr = f[..., 7] != 0
    cand = np.where(ovr, np.maximum(b00, np.minimum(b10, cap)),
                    np.where(2 * a_d - 1 > 0, head_wait, head_cross).astype(np.float64))
    a = np.full((M, S), b10)
    binds = np.zeros((M, S, P), bool)
    for p in range(P):
        a = np.where(cand[:, :, p] < a, cand[:, :, p], a)
        binds[:, :, p] = cap[:, :, p] < a
        a = np.where(cap[:, :, p] < a, cap[:, :, p], a)
    lights = 2.0 * a_d.reshape(M, S * P)[:, :S] - 1.0
    reg = dict(at_b00=ovr & (cap < b00), at_b10=ovr & (cap > b10), between=ovr & (cap > b00) & (cap < b10),
               cap_binds=binds)
    return np.concatenate([a, lights], 1), reg


def policy_reference(hp, hf, cfg, c, w, rows):
    """rows [M, od] of the env at cfg -> (the rows with redrawn speeds, the host build's decisions a_d, the
    features, policy_act_ref's actions and regimes); hp / hf: tools/hostpolicy and tools/hostfwd, c the host
    policy's config, w the packed (cross, wait, choice) weights of actors with mean -1 and std 3."""
    obs = speed_rows(rows, hp.dims(c)[1], cfg)
    a_d = hp.decide(c, w[2], obs)
    f = hp.features(c, obs)
    heads = [hf.forward(1, w[k], f.reshape(-1, 13), -1.0, 3.0).reshape(f.shape[:3]) for k in (0, 1)]
    ref, reg = policy_act_ref(f, a_d, heads[0], heads[1], cfg)
    return obs, a_d, f, ref, reg
