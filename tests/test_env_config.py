"""The C env oracle and the device env source (compiled for the CPU, tools/hostsim) away from
the default env configuration (dt 0.3, 80 steps, the sin pedestrian model, the standard bounds).

Fixtures: tests/golden/envcfg_<shape>_<A|B|C|D>.npz, recorded from the reference envs by
tests/golden/gen/make_env_golden.py at the four configurations of envcfg_common.CONFIGS (the
uniform pedestrian model, other dt / max_episode, bounds whose braking distance divides by a
non-power-of-two).  Both restatements replay them bit for bit, detection's print counts
included, and agree with each other bit for bit on every configuration x shape x env view.
With host libm on both sides this pins the logic; tests/test_env_config_gpu.py then only has
device-libm ulps to account for.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import envcfg_common as ec
import oracle
from oracle import OracleBatch, OracleEnv, env_kwargs

ROOT = ec.ROOT


@pytest.fixture(scope="module")
def hostsim():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools")])
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import hostsim as hs
    return hs


def test_fixture_set_covers_every_config_and_variant():
    cfgs, variants, multi_ped = set(), set(), False
    for f in ec.FILES:
        g = np.load(f)
        assert os.path.getsize(f) <= 245760 and g["obs"].shape[0] == 6
        c = ec.fixture_cfg(g)
        cid = os.path.basename(f)[:-4].rsplit("_", 1)[1]
        ref = {**ec.DEFAULT, **ec.CONFIGS[cid]}
        assert (c["dt"], c["max_episode"], c["simulation"]) == (ref["dt"], ref["max_episode"], ref["simulation"])
        for k, d in (("car_b", oracle.CAR_B), ("ped_b", oracle.PED_B), ("cross_b", oracle.CROSS_B)):
            assert np.array_equal(c[k], np.asarray(ref.get(k, d), dtype=np.float64)), (f, k)
        assert g["obs"].shape[1] > c["max_episode"]  # stepped past done
        cfgs.add(cid)
        variants.add(str(g["variant"]))
        multi_ped |= int(g["nb_ped"]) > 1
    assert cfgs == set("ABCD") and variants == {"coop", "4cars", "scalable", "naif", "4cars2", "stop"} and multi_ped


@pytest.mark.parametrize("path", ec.FILES, ids=ec.FILE_IDS)
def test_oracle_replays_config_fixture(path):
    g = np.load(path)
    v = str(g["variant"])
    nc, npd, nl = int(g["nb_car"]), int(g["nb_ped"]), int(g["nb_lines"])
    E, T = g["obs"].shape[:2]
    kw = env_kwargs(ec.fixture_cfg(g))
    ev = np.cumsum(g["events"].astype(np.int64), axis=1)
    for e in range(E):
        env = OracleEnv(v, nc, npd, nl, seed=int(g["seed_base"]) + e, **kw)
        o = env.reset()
        assert np.array_equal(o, g["obs0"][e]), f"reset obs env {e}"
        assert env.rng_state()[1] % 624 == g["mti0"][e] % 624
        for t in range(T):
            o, r, rl, d = env.step(g["actions"][e, t])
            ctx = f"env {e} step {t}"
            assert np.array_equal(o, g["obs"][e, t]), ctx
            assert np.array_equal(r, g["rewards"][e, t]), ctx
            assert np.array_equal(rl, g["reward_light"][e, t]), ctx
            assert d == bool(g["done"][e, t]), ctx
            assert env.rng_state()[1] % 624 == g["mti"][e, t] % 624, ctx
            assert np.array_equal(env.dump(), g["dump"][e, t]), ctx
            assert np.array_equal(env.events(), ev[e, t]), ctx
        mt, _ = env.rng_state()
        assert np.array_equal(mt, g["final_mt"][e])


@pytest.mark.parametrize("view", ["default", "generic"])
@pytest.mark.parametrize("path", ec.FILES, ids=ec.FILE_IDS)
def test_device_source_replays_config_fixture(hostsim, path, view):
    g = np.load(path)
    E, T = g["obs"].shape[:2]
    h = hostsim.HostVec(str(g["variant"]), E, int(g["nb_car"]), int(g["nb_ped"]), int(g["nb_lines"]),
                        seed_base=int(g["seed_base"]), flags=2 if view == "generic" else 0, **ec.fixture_cfg(g))
    assert np.array_equal(h.reset(), g["obs0"])
    assert not h.events().any()
    ev = np.cumsum(g["events"].astype(np.int64), axis=1)
    k = g["dump"].shape[2]
    for t in range(T):
        o, r, rl, d = h.step(g["actions"][:, t])
        assert np.array_equal(o, g["obs"][:, t]), t
        assert np.array_equal(r, g["rewards"][:, t]), t
        assert np.array_equal(rl, g["reward_light"][:, t]), t
        assert np.array_equal(d, g["done"][:, t]), t
        assert np.array_equal(h.state()[:, :k], g["dump"][:, t]), t
        assert np.array_equal(h.events(), ev[:, t]), t


@pytest.mark.parametrize("view", ["default", "generic"])
@pytest.mark.parametrize("shape", ec.SHAPES, ids=ec.shape_id)
@pytest.mark.parametrize("cid", sorted(ec.CONFIGS))
def test_device_source_matches_oracle_at_config(hostsim, cid, shape, view):
    """64 envs, one episode and five steps past its end: observations, rewards, reward_light,
    done, the internal state and the event counters, bit for bit."""
    cfg = ec.CONFIGS[cid]
    v, nc, npd, nl = shape
    N, T = 64, cfg["max_episode"] + 5
    h = hostsim.HostVec(v, N, nc, npd, nl, seed_base=4100, flags=2 if view == "generic" else 0, **cfg)
    orc = OracleBatch(v, N, nc, npd, nl, seed_base=4100, **env_kwargs(cfg))
    assert np.array_equal(h.reset(), orc.reset())
    acts = ec.action_stream(cfg, N, orc.A, T)
    k = orc.dump_dim
    for t in range(T):
        o, r, rl, d = h.step(acts[t])
        oo, ro, rlo, do, dm, _ = orc.step(acts[t], want_dump=True)
        assert np.array_equal(o, oo), t
        assert np.array_equal(r, ro), t
        assert np.array_equal(rl, rlo), t
        assert np.array_equal(d, do), t
        assert np.array_equal(h.state()[:, :k], dm), t
        assert np.array_equal(h.events(), orc.events()), t


@pytest.mark.parametrize("view", ["default", "generic"])
@pytest.mark.parametrize("max_episode,dt,first_done", [(25, 0.5, 24), (50, 0.3, 49), (50, 0.5, 49), (50, 0.2, 50)])
def test_done_is_raised_at_max_episode(hostsim, max_episode, dt, first_done, view):
    """done at step max_episode - 1 and at no earlier step, in the oracle and in the device source.

    The reference raises done when time >= (max_episode - 1) * dt with time accumulated by repeated
    `time + dt` in float64 (Env_hybrid_multi_coop.py:892).  At dt 0.2 the sum of 49 steps is
    9.799999999999997 < 49 * 0.2, so the reference plays 51 steps at max_episode 50 (config B; the
    envcfg_*_B fixtures recorded from it show the same): that case pins the accumulation itself."""
    time, t = 0.0, 0
    while not time >= (max_episode - 1) * dt:
        time, t = time + dt, t + 1
    assert t == first_done
    cfg = dict(dt=dt, max_episode=max_episode, simulation="unif")
    N = 16
    h = hostsim.HostVec("coop", N, 2, 1, 2, seed_base=77, flags=2 if view == "generic" else 0, **cfg)
    orc = OracleBatch("coop", N, 2, 1, 2, seed_base=77, **env_kwargs(cfg))
    h.reset()
    orc.reset()
    acts = ec.action_stream(cfg, N, 2, first_done + 1)
    for t in range(first_done + 1):
        want = t == first_done
        assert (h.step(acts[t])[3] == want).all(), t
        assert (orc.step(acts[t])[3] == want).all(), t


def test_oracle_batch_steps_4cars2():
    """OracleBatch takes 4cars2's 2 * nb_car action slots (AVs and followers) and equals OracleEnv."""
    N, nc = 5, 4
    orc = OracleBatch("4cars2", N, nc, 1, 2, seed_base=31)
    one = [OracleEnv("4cars2", nc, 1, 2, seed=31 + e) for e in range(N)]
    assert orc.A == 2 * nc and orc.S == nc
    assert np.array_equal(orc.reset(), np.stack([o.reset() for o in one]))
    acts = ec.action_stream({}, N, orc.A, 20)
    for t in range(20):
        got = orc.step(acts[t])
        ref = [o.step(acts[t][e]) for e, o in enumerate(one)]
        for j in range(3):
            assert np.array_equal(got[j], np.stack([x[j] for x in ref])), (t, j)



def _policy_case(pid, shape, mean):
    """Host policy config, packed random-init weights (cross, wait, choice) and dims of a POLICY_CFGS case."""
    import torch
    from mhppo.models import Model_PPO
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import hostpolicy as hp
    cfg = ec.POLICY_CFGS[pid]
    c = hp.cfg(*shape, dt=cfg["dt"], car_b=cfg["car_b"])
    dims = hp.dims(c)
    torch.manual_seed(7)
    w = [Model_PPO(13, 1, 1).packed().numpy(), Model_PPO(13, 1, 1).packed().numpy(),
         Model_PPO(dims[3], 2, 2).packed().numpy()]
    return hp, cfg, c, dims, w


POLICY_SHAPES = [("coop", 2, 1, 2), ("scalable", 4, 2, 2), ("stop", 2, 2, 2)]


@pytest.mark.parametrize("shape", POLICY_SHAPES, ids=ec.shape_id)
@pytest.mark.parametrize("pid", sorted(ec.POLICY_CFGS))
def test_host_policy_equals_oracle_evaluate_at_config(pid, shape):
    """The stateless policy's rule (csrc/policy_rule.h compiled for the CPU) on the observation rows of
    oracle.evaluate at a non-default dt and car_b reproduces the oracle's actions bit for bit.  The
    actors' mean is +1 so that the cars reach the speed limit: the (10 - V) / dt cap must bind and a
    left-lane override must occur, and the default dt / bounds must not pass."""
    hp, cfg, c, (od, S, P, dc), w = _policy_case(pid, shape, 1.0)
    variant, nb_car, nb_ped, nb_lines = shape
    T, E, K = cfg["max_episode"], 8, 2
    res = oracle.evaluate(variant, nb_car, nb_ped, nb_lines, [4242 + e for e in range(E)], K, *w, mean=1.0, T=T,
                          env_cfg=cfg)
    obs = np.concatenate([r["obs"] for r in res])
    ref = np.concatenate([r["acts"] for r in res])
    assert obs.shape == (E * K * T, od)
    # the decisions in force at each row: re-decided at an episode's first row and when the test fires
    col = obs[:, od - 9 * P - (4 if variant == "scalable" else 3) + 1]
    due = np.zeros(len(obs), bool)
    due[1:] = (col[1:] != np.float32(P)) if variant == "scalable" else (col[1:] != col[:-1])
    due[::T] = True
    a_d = hp.decide(c, w[2], obs)[np.maximum.accumulate(np.where(due, np.arange(len(obs)), 0))]
    acts = hp.act(c, w[0], w[1], obs, a_d, mean=1.0)[:, :S]
    assert np.array_equal(acts.astype(np.float32).view(np.uint32), ref.view(np.uint32))
    f = hp.features(c, obs)
    cap = (10.0 - f[..., 0].astype(np.float64)) / cfg["dt"]
    assert ((acts[:, :, None] == cap) & (f[..., 7] == 0)).any(), "the speed cap binds nowhere"
    assert (f[..., 7] != 0).any(), "no left-lane row"
    default = hp.act(hp.cfg(variant, nb_car, nb_ped, nb_lines), w[0], w[1], obs, a_d, mean=1.0)[:, :S]
    assert not np.array_equal(default, acts)


@pytest.mark.parametrize("shape", POLICY_SHAPES, ids=ec.shape_id)
@pytest.mark.parametrize("pid", sorted(ec.POLICY_CFGS))
def test_host_policy_rule_near_the_speed_limit(hostsim, pid, shape):
    """Rows of the env at the configuration with car speeds redrawn around 10 (envcfg_common.speed_rows): the
    override clamps at car_b[0][0], at car_b[1][0] and strictly between, the cap binds, and the host build
    of the rule equals its plain float64 restatement (envcfg_common.policy_act_ref) bit for bit."""
    import infer_common as ic
    hp, cfg, c, (od, S, P, dc), w = _policy_case(pid, shape, -1.0)
    obs, a_d, f, ref, reg = policy_rows(hostsim, hp, ic.hostfwd(), cfg, c, shape, w)
    for k, m in reg.items():
        assert m.any(), f"no row where {k}"
    assert np.array_equal(hp.act(c, w[0], w[1], obs, a_d).view(np.uint64), ref.view(np.uint64))


def policy_rows(hostsim, hp, hf, cfg, c, shape, w, n_envs=16, steps=40):
    """ec.policy_reference on the rows of n_envs host-built envs at the configuration over `steps` steps."""
    variant, nb_car, nb_ped, nb_lines = shape
    h = hostsim.HostVec(variant, n_envs, nb_car, nb_ped, nb_lines, seed_base=20, **cfg)
    rows = [h.reset()]
    for a in ec.action_stream(cfg, n_envs, hp.dims(c)[1], steps - 1, seed=20):
        rows.append(h.step(a)[0])
    return ec.policy_reference(hp, hf, cfg, c, w, np.concatenate(rows))
