"""The HIP env, the rollout collector, the evaluation and the stateless policy away from the default
env configuration (dt 0.3, 80 steps, the sin pedestrian model, the standard bounds).

Configurations A-D (envcfg_common.CONFIGS): the uniform pedestrian model (the facade's default), other
dt / max_episode, and bounds B2 whose -2 * car_b[0][0] = 6 is no power of two, so the braking distance
takes its true division (env_body.h build_cfg, brake_p2).  tests/test_env_config.py pins the env's
logic at the same configurations on the CPU (the device source with host libm, bit for bit); what is
left here is the device build: device libm, the register view's specialisations, the brake division,
and every GPU consumer of dt / car_b / max_episode.

Tolerances are the project's: RNG streams, done flags, discrete fields and event counters exact;
float32 observations 1e-6; float64 rewards / state rtol 1e-9, atol 1e-12; the collector's are those of
tests/test_rollout_gpu.py, the evaluation's those of tests/test_oracle_eval.py.

The share of float64 rewards / reward_light whose last bits differ from glibc is printed per case and
not capped (every value is held to 1e-9).  Measured on an MI355X, N = 512, one episode:
    config   coop 2/1/2  coop 4/3/2  4cars 4/1/2  scalable 8/1/4  scalable 4/3/2  naif 1/1/1  stop 2/2/2
    A        1.12 %      0.79 %      0.68 %       0.82 %          0.67 %          0.44 %      0.57 %
    D        2.71 %      2.53 %      2.70 %       1.40 %          1.32 %          2.70 %      3.10 %
    B        1.03 %      -           -            0.84 %          -               -           -
    C        0.94 %      -           -            0.76 %          -               -           -
    default  stop 2/1/2: 0.58 %, 4cars2 4/1/2: 0.69 %
"""
import os
import sys

import numpy as np
import pytest
import torch

import envcfg_common as ec

ROOT = ec.ROOT
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu
DISCRETE_PED = [4, 5, 6, 7, 8, 9, 10, 11, 17, 18, 19]  # per-ped dump fields that are flags / ints
DISCRETE_CAR = [3, 7]  # light, exist


@pytest.mark.parametrize("view", ["default", "generic"])
@pytest.mark.parametrize("path", ec.FILES, ids=ec.FILE_IDS)
def test_gpu_env_replays_config_fixture(path, view):
    from mhppo.env import VecCrosswalk
    g = np.load(path)
    E, T = g["obs"].shape[:2]
    npd = int(g["nb_ped"])
    env = VecCrosswalk(str(g["variant"]), E, int(g["nb_car"]), npd, int(g["nb_lines"]), seed_base=int(g["seed_base"]),
                       generic_step=view == "generic", **ec.fixture_cfg(g))
    assert np.array_equal(env.reset().cpu().numpy(), g["obs0"])
    assert not env.events().any()
    ev = np.cumsum(g["events"].astype(np.int64), axis=1)  # detection's prints per env and step, as the reference printed
    k = g["dump"].shape[2]
    for t in range(T):
        o, r, rl, d = env.step(torch.from_numpy(g["actions"][:, t]).cuda())
        assert np.array_equal(env.events().cpu().numpy(), ev[:, t]), t
        st = env.get_state().cpu().numpy()[:, :k]
        ref = g["dump"][:, t]
        assert np.array_equal(d.cpu().numpy(), g["done"][:, t])
        np.testing.assert_allclose(o.cpu().numpy(), g["obs"][:, t], rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(r.cpu().numpy(), g["rewards"][:, t], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(rl.cpu().numpy(), g["reward_light"][:, t], rtol=1e-9, atol=1e-12)
        ped = st[:, :20 * npd].reshape(E, npd, 20)[:, :, DISCRETE_PED]
        assert np.array_equal(ped, ref[:, :20 * npd].reshape(E, npd, 20)[:, :, DISCRETE_PED]), t
        np.testing.assert_allclose(st, ref, rtol=1e-9, atol=1e-12)
    mt, _ = env.get_rng()
    assert np.array_equal(mt.cpu().numpy().view(np.uint32), g["final_mt"])


MANY = ([(c, s) for c in "AD" for s in ec.SHAPES] +
        [(c, s) for c in "BC" for s in (("coop", 2, 1, 2), ("scalable", 8, 1, 4))] +
        [("default", ("stop", 2, 1, 2)), ("default", ("4cars2", 4, 1, 2))])


@pytest.mark.parametrize("cid,shape", MANY, ids=[f"{c}-{ec.shape_id(s)}" for c, s in MANY])
def test_gpu_env_matches_oracle_at_config(cid, shape):
    """512 envs over one episode (max_episode steps) against the C oracle, every step and every env: exactly
    done, the RNG cursor, the discrete pedestrian and car fields and the event counters, at the end the
    whole MT19937 state; the continuous outputs to the project's tolerances."""
    from mhppo.env import VecCrosswalk
    from oracle import OracleBatch, env_kwargs, set_threads
    set_threads(min(16, os.cpu_count() or 1))
    cfg = ec.CONFIGS.get(cid, ec.DEFAULT)
    v, nc, npd, nl = shape
    N, T, seed = 512, cfg["max_episode"], 9000
    env = VecCrosswalk(v, N, nc, npd, nl, seed_base=seed, **cfg)
    orc = OracleBatch(v, N, nc, npd, nl, seed_base=seed, **env_kwargs(cfg))
    assert env.n_slots == orc.A and env.n_reward_slots == orc.S
    assert np.array_equal(env.reset().cpu().numpy(), orc.reset())
    k = orc.dump_dim
    acts = ec.action_stream(cfg, N, orc.A, T)
    n_diff = n_tot = 0
    for t in range(T):
        o, r, rl, d = env.step(torch.from_numpy(acts[t]).cuda())
        st = env.get_state()[:, :k].cpu().numpy()
        _, mti_g = env.get_rng()
        o, r, rl, d = o.cpu().numpy(), r.cpu().numpy(), rl.cpu().numpy(), d.cpu().numpy()
        oo, ro, rlo, do, dm, mti_o = orc.step(acts[t], want_dump=True)
        assert np.array_equal(d, do), t
        assert np.array_equal(mti_g.cpu().numpy(), mti_o), t
        for fields, lo, hi, w in ((DISCRETE_PED, 0, 20 * npd, 20), (DISCRETE_CAR, 20 * npd, k, 8)):
            assert np.array_equal(st[:, lo:hi].reshape(N, -1, w)[:, :, fields],
                                  dm[:, lo:hi].reshape(N, -1, w)[:, :, fields]), (t, w)
        assert np.array_equal(env.events().cpu().numpy().astype(np.uint32), orc.events()), t
        np.testing.assert_allclose(o, oo, rtol=1e-6, atol=1e-6, err_msg=str(t))
        np.testing.assert_allclose(r, ro, rtol=1e-9, atol=1e-12, err_msg=str(t))
        np.testing.assert_allclose(rl, rlo, rtol=1e-9, atol=1e-12, err_msg=str(t))
        np.testing.assert_allclose(st, dm, rtol=1e-9, atol=1e-12, err_msg=str(t))
        n_diff += int((r != ro).sum() + (rl != rlo).sum())
        n_tot += r.size + rl.size
    mt_g, _ = env.get_rng()
    assert np.array_equal(mt_g.cpu().numpy().view(np.uint32), orc.rng_state()[0])
    # reported, not capped: every value above is held to 1e-9
    print(f"config {cid} {ec.shape_id(shape)}: {n_diff}/{n_tot} = {n_diff / n_tot:.4%} float64 rewards differ "
          "in their last bits")


@pytest.mark.parametrize("shape", [("coop", 2, 1, 2), ("scalable", 8, 1, 4), ("stop", 2, 1, 2)], ids=ec.shape_id)
@pytest.mark.parametrize("cid", ["C", "D"])
def test_register_view_is_bit_identical_to_generic_at_config(cid, shape):
    """The register env view and the in-HBM view over two episodes (the second starts without a reset)."""
    from mhppo.env import VecCrosswalk
    cfg = ec.CONFIGS[cid]
    v, nc, npd, nl = shape
    N, T = 1024, 2 * cfg["max_episode"]
    envs = [VecCrosswalk(v, N, nc, npd, nl, seed_base=777, generic_step=g, **cfg) for g in (False, True)]
    o0 = [e.reset() for e in envs]
    assert torch.equal(o0[0], o0[1])
    acts = torch.from_numpy(ec.action_stream(cfg, N, envs[0].n_slots, T, seed=4)).cuda()
    for t in range(T):
        outs = [e.step(acts[t]) for e in envs]
        for x, y in zip(outs[0], outs[1]):
            assert torch.equal(x, y), t
    assert torch.equal(envs[0].get_state(), envs[1].get_state())
    assert torch.equal(envs[0].events(), envs[1].events())
    (m0, i0), (m1, i1) = envs[0].get_rng(), envs[1].get_rng()
    assert torch.equal(m0, m1) and torch.equal(i0, i1)


@pytest.mark.parametrize("shape", [("coop", 2, 1, 2), ("scalable", 8, 1, 4), ("stop", 2, 2, 2)], ids=ec.shape_id)
@pytest.mark.parametrize("cid", ["B", "D"])
def test_gpu_rollout_matches_oracle_at_config(cid, shape):
    """RolloutGPU.collect with T = max_episode against oracle.rollout: the assertions and tolerances of
    tests/test_rollout_gpu.py::test_gpu_rollout_matches_oracle_philox."""
    import oracle
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    from mhppo.rollout import RolloutGPU
    cfg = ec.CONFIGS[cid]
    v, nc, npd, nl = shape
    N = 256
    venv = VecCrosswalk(v, N, nc, npd, nl, seed_base=31000, **cfg)
    ro = RolloutGPU(venv)
    assert ro.T == cfg["max_episode"]
    torch.manual_seed(5)
    ac = Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda()
    aw = Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda()
    ad = Model_PPO(ro.dc, 2, 2).cuda()
    batch = ro.collect(ac, aw, ad, seed=3, iteration=0)
    go = {k: getattr(batch, k).cpu().numpy() for k in ("feat_d", "a_d", "logp_d", "closest", "exist", "obs_c", "act",
                                                       "logp", "rew", "ep_min")}
    o = oracle.rollout(v, nc, npd, nl, [31000 + e for e in range(N)], ac.packed().cpu().numpy(),
                       aw.packed().cpu().numpy(), ad.packed().cpu().numpy(), u=ro.u.cpu().numpy(),
                       eps=ro.eps.cpu().numpy(), T=ro.T, env_cfg=cfg)
    assert go["act"].shape == o["act"].shape == (N, venv.n_slots, cfg["max_episode"])
    for k in ("a_d", "closest", "exist"):
        np.testing.assert_array_equal(go[k], o[k], err_msg=k)
    np.testing.assert_allclose(go["feat_d"], o["feat_d"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(go["logp_d"], o["logp_d"], rtol=1e-5, atol=1e-5)
    m = go["exist"].astype(bool)
    assert batch.rec_of is not None or m.all()
    np.testing.assert_allclose(go["obs_c"][m], o["obs_c"][m], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(go["act"][m], o["act"][m], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(go["logp"][m], o["logp"][m], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(go["rew"][m], o["rew"][m], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(go["ep_min"], o["ep_min"], rtol=1e-5, atol=1e-5)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("shape", [("coop", 2, 1, 2), ("scalable", 4, 2, 2), ("stop", 2, 2, 2)], ids=ec.shape_id)
@pytest.mark.parametrize("pid", sorted(ec.POLICY_CFGS))
def test_policy_bits_equal_host_build_at_config(pid, shape):
    """Policy(..., dt=, car_b=).act and .sample_act on 640 rows of the env at the configuration, car speeds
    redrawn around 10 (envcfg_common.speed_rows): bit for bit the host build of the rule (tools/hostpolicy),
    which tests/test_env_config.py holds to the oracle and to a plain float64 restatement.  The rows must
    hold a left-lane override clamped at car_b[0][0], at car_b[1][0] and strictly between, and a binding cap."""
    import hostpolicy as hp
    import infer_common as ic
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    from mhppo.policy import Policy
    cfg = ec.POLICY_CFGS[pid]
    variant, nb_car, nb_ped, nb_lines = shape
    c = hp.cfg(variant, nb_car, nb_ped, nb_lines, dt=cfg["dt"], car_b=cfg["car_b"])
    od, S, P, dc = hp.dims(c)
    torch.manual_seed(7)
    ac, aw = (Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda() for _ in range(2))
    ad = Model_PPO(dc, 2, 2).cuda()
    w = [n.packed().cpu().numpy() for n in (ac, aw, ad)]
    n_envs, steps = 16, 40
    venv = VecCrosswalk(variant, n_envs, nb_car, nb_ped, nb_lines, seed_base=20, **cfg)
    rows = [venv.reset()]
    for a in ec.action_stream(cfg, n_envs, S, steps - 1, seed=20):
        rows.append(venv.step(torch.from_numpy(a).cuda())[0])
    obs_np, a_d, f, ref, reg = ec.policy_reference(hp, ic.hostfwd(), cfg, c, w, torch.cat(rows).cpu().numpy())
    for k, m in reg.items():
        assert m.any(), f"no row where {k}"
    host = hp.act(c, w[0], w[1], obs_np, a_d)
    assert same_bits(host, ref)
    obs = torch.from_numpy(obs_np).cuda()
    for pol in (Policy(variant, nb_car, nb_ped, nb_lines, ac, aw, ad, dt=cfg["dt"], car_b=cfg["car_b"]),
                Policy.from_env(venv, ac, aw, ad)):
        assert (pol.obs_dim, pol.n_slots, pol.nb_ped, pol.choice_dim) == (od, S, P, dc)
        got_d = pol.decide(obs)
        assert same_bits(got_d.cpu().numpy(), a_d)
        assert same_bits(pol.act(obs, got_d).cpu().numpy(), host)
    # the default dt / bounds give other actions on these rows: the comparison sees the configuration
    assert not same_bits(Policy(variant, nb_car, nb_ped, nb_lines, ac, aw, ad).act(obs, got_d).cpu().numpy(), host)
    # the stochastic rule (no cap, no override: it must not depend on the configuration either way)
    rng = np.random.default_rng(5)
    u = rng.uniform(size=(len(obs_np), S, P)).astype(np.float32)
    eps = rng.normal(size=(len(obs_np), S)).astype(np.float32)
    hd = hp.sample_decide(c, w[2], obs_np, u=u)
    ha = hp.sample_act(c, w[0], w[1], obs_np, hd["a_d"], hd["closest"], eps=eps)
    assert hd["status"] == 0 and ha["status"] == 0
    d = pol.sample_decide(obs, u=torch.from_numpy(u).cuda())
    assert same_bits(d.a_d.cpu().numpy(), hd["a_d"]) and same_bits(d.closest.cpu().numpy(), hd["closest"])
    assert same_bits(d.exist.cpu().numpy(), hd["exist"])
    np.testing.assert_allclose(d.logp_d.cpu().numpy(), hd["logp_d"], rtol=1e-5, atol=1e-5)
    r = pol.sample_act(obs, d.a_d, d.closest, eps=torch.from_numpy(eps).cuda())
    for name in ("actions", "act", "logp", "feat_c"):
        assert same_bits(getattr(r, name).cpu().numpy(), ha[name]), name


def test_algo_evaluate_matches_oracle_at_config():
    """Algo_PPO.evaluate(2) at config D (dt 0.5, 25 steps, uniform pedestrians, B2 bounds: the actors' mean
    and std, the clamp and the cap all follow the configuration) against oracle.evaluate, 64 scalable envs."""
    import oracle
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    from test_oracle_eval import check_eval
    cfg = ec.CONFIGS["D"]
    N, K, T = 64, 2, cfg["max_episode"]
    torch.manual_seed(7)
    venv = VecCrosswalk("scalable", N, 4, 2, 2, seed_base=4242, **cfg)
    algo = Algo_PPO(Model_PPO, venv, verbose=False)
    assert (algo.mean, algo.std, algo.max_steps) == (-0.75, 2.25, T)
    w = [n.packed().cpu().numpy() for n in (algo.actor_net_cross, algo.actor_net_wait, algo.actor_net_choice)]
    out = dict(zip(("obs", "acts", "rews_c", "rews_d", "waiting"), (x.cpu().numpy() for x in algo.evaluate(K))))
    assert out["obs"].shape == (N * K * T, venv.obs_dim)
    res = oracle.evaluate("scalable", 4, 2, 2, [4242 + e for e in range(N)], K, *w, mean=algo.mean, std=algo.std, T=T,
                          env_cfg=cfg, resets=2)
    check_eval(out, {k: np.concatenate([r[k] for r in res]) for k in res[0]})


def test_evaluate_stats_matches_get_average_at_50_steps():
    """evaluate_stats(2) == get_average(evaluate(2)[0]) at max_episode = 50, under the comparison of
    tests/test_evalstats_gpu.py::test_evaluate_stats_matches_get_average."""
    from evalstats_common import check_dict
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    from mhppo.stats import get_average
    n, K = 8, 2
    algos = []
    for _ in range(2):
        torch.manual_seed(1234)
        algos.append(Algo_PPO(Model_PPO, VecCrosswalk("coop", n, 2, 1, 2, seed_base=77, max_episode=50,
                                                      simulation="unif"), verbose=False))
    ref_algo, algo = algos
    states = ref_algo.evaluate(K)[0]
    assert states.shape[0] == n * K * 50
    ref = get_average(states.cpu(), "coop", 2, 1, 2)
    assert ref["episodes"] == n * K  # precondition: the equal-width runs are the true episodes
    got = algo.evaluate_stats(K)
    assert set(got) == set(ref)
    check_dict(got, ref)
    a, b = ref_algo.venv.state_dict(), algo.venv.state_dict()
    assert a["cfg"] == b["cfg"] and torch.equal(a["blob"], b["blob"])


def test_facade_default_is_the_uniform_model():
    """envs.make(id, ...) without simulation= runs the uniform pedestrian model, as the reference's envs
    do: it steps like the oracle with sin=False and unlike the sin trajectory."""
    import oracle
    from mhppo import envs
    kw = dict(car_b=oracle.CAR_B, ped_b=oracle.PED_B, cross_b=oracle.CROSS_B, nb_car=2, nb_ped=1, nb_lines=2, dt=0.3,
              max_episode=80)
    env = envs.make("Crosswalk_hybrid_multi_coop-v0", **kw)
    assert env.simulation == "unif"
    unif, sin = (oracle.OracleEnv("coop", 2, 1, 2, seed=10, sin=s) for s in (False, True))  # the facade's seed
    flat = lambda s: np.concatenate([np.ravel(v) for v in s.values()])
    o0 = flat(env.reset()[0])
    assert np.array_equal(o0, unif.reset())
    sin.reset()
    acts = ec.action_stream({}, 1, 2, 80, seed=6)[:, 0]
    differs = False
    for t in range(80):
        s, r, d, _, _ = env.step(acts[t])
        ou, ru, rlu, du = unif.step(acts[t])
        assert d == du, t
        np.testing.assert_allclose(flat(s), ou, rtol=1e-6, atol=1e-6, err_msg=str(t))
        np.testing.assert_allclose(r, ru, rtol=1e-9, atol=1e-12, err_msg=str(t))
        np.testing.assert_allclose(env.reward_light, rlu, rtol=1e-9, atol=1e-12, err_msg=str(t))
        differs |= not np.allclose(ou, sin.step(acts[t])[0], rtol=1e-6, atol=1e-6)
    assert differs
