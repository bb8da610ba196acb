"""The stochastic policy's rule (csrc/policy_sample_rule.h, compiled for the CPU: tools/hostpolicy.py)
against the C oracle's rollout on the rollout fixtures' weights and recorded draws: an oracle env is
stepped with the actions the rule computes from its observation rows, and every record the oracle's own
rollout keeps (oracle.OracleBatch.rollout: feat_d, probs, closest, exist, then per step act, logp, obs_c
and the rewards its applied action earns) is reproduced bit for bit on every slot, absent cars' included;
logp_d within the
tolerance tests/test_rollout_gpu.py uses between two logf.  And the in-rule Philox noise against
tests/philox_ref.py at the collector's counters."""
import os
import sys

import numpy as np
import pytest

import philox_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FIXTURES = ["rollout_coop_422", "rollout_naif_111", "rollout_scalable_422", "rollout_scalable_814"]
T = 80


def _hp():
    import hostpolicy
    return hostpolicy


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", FIXTURES)
def test_rule_replays_oracle_rollout(name):
    import oracle
    hp = _hp()
    g = np.load(os.path.join(ROOT, "tests", "golden", f"{name}.npz"))
    variant, shape = str(g["variant"]), (int(g["nb_car"]), int(g["nb_ped"]), int(g["nb_lines"]))
    eps, a_d, seed = g["eps"], g["a_d"], int(g["seed_base"])
    N = a_d.shape[0]
    c = hp.cfg(variant, *shape)
    od, S, P, dc = hp.dims(c)
    assert eps.shape == (T, N, S) and a_d.shape == (N, S, P)
    w = [g["w_cross"], g["w_wait"], g["w_choice"]]
    ref = oracle.OracleBatch(variant, N, *shape, seed_base=seed).rollout(*w, forced_a=a_d, eps=eps, T=T)
    env = oracle.OracleBatch(variant, N, *shape, seed_base=seed)
    obs = env.reset()
    d = hp.sample_decide(c, w[2], obs, forced=a_d)
    assert d["status"] == 0
    assert bits(d["a_d"], a_d) and bits(d["feat_d"], ref["feat_d"]) and bits(d["probs"], ref["probs_d"])
    assert bits(d["closest"], ref["closest"]) and bits(d["exist"], ref["exist"])
    np.testing.assert_allclose(d["logp_d"], ref["logp_d"], rtol=1e-5, atol=1e-5)
    present = ref["exist"].astype(bool)  # [N, S]
    if variant == "scalable":
        assert (~present).any() and present.any()
    alive = np.ones(N, bool)
    sel_moved = False
    for t in range(T):
        r = hp.sample_act(c, w[0], w[1], obs, a_d, d["closest"], eps=eps[t])
        assert r["status"] == 0
        # every slot of a running episode: the oracle computes, records and applies an absent car's action
        # like any other (it reaches present slots' rewards), and so does the rule
        m = np.broadcast_to(alive[:, None], present.shape)
        assert bits(r["act"][m], ref["act"][:, :, t][m]), t
        assert bits(r["logp"][m], ref["logp"][:, :, t][m]), t
        assert bits(r["feat_c"][m], ref["obs_c"][:, :, t][m]), t
        assert bits(r["actions"][:, :S][m], ref["act"][:, :, t][m].astype(np.float64)), t
        lights = 2.0 * np.take_along_axis(a_d, d["closest"][:, :, None], 2)[:, :, 0] - 1.0
        assert bits(r["actions"][:, S:], lights), t
        sel_moved |= P > 1 and not bits(r["feat_c"], hp.features(c, obs)[:, :, 0])
        obs, rew, rl, done, _, _ = env.step(r["actions"])
        # the applied action: the oracle's own rollout earned these rewards with it
        assert bits(rew[m], ref["rew"][:, :, t][m]), t
        alive &= ~done  # the oracle's rollout stops an env's episode at `done`
        if not alive.any():
            break
    if P > 1:
        assert sel_moved, "no slot selected a pedestrian other than the first"


def test_forced_and_uniform_draws_agree():
    """a_d = u >= n[0]: forcing the decisions a uniform tape draws gives the tape's outputs back."""
    import oracle
    hp = _hp()
    g = np.load(os.path.join(ROOT, "tests", "golden", "rollout_coop_422.npz"))
    c = hp.cfg("coop", 4, 2, 2)
    obs = oracle.OracleBatch("coop", 4, 4, 2, 2, seed_base=3).reset()
    u = np.random.default_rng(1).uniform(size=(4, 4, 2)).astype(np.float32)
    a = hp.sample_decide(c, g["w_choice"], obs, u=u)
    n0 = a["probs"][..., 0] / (a["probs"][..., 0] + a["probs"][..., 1])
    assert np.array_equal(a["a_d"], (u >= n0).astype(np.int32)) and 0 < a["a_d"].sum() < a["a_d"].size
    b = hp.sample_decide(c, g["w_choice"], obs, forced=a["a_d"])
    for k in ("a_d", "logp_d", "probs", "feat_d", "closest", "exist"):
        assert bits(a[k], b[k]), k
    with pytest.raises(ValueError):
        hp.sample_decide(c, g["w_choice"], obs, u=u, forced=a["a_d"])
    with pytest.raises(ValueError):
        hp.sample_decide(c, g["w_choice"], obs)


@pytest.mark.parametrize("shape,first_env,t", [(("coop", 4, 2, 2), 0, 0), (("scalable", 8, 3, 4), 7, 0),
                                               (("scalable", 8, 3, 4), 2**33 + 5, 79), (("naif", 1, 1, 1), 1000, 3)],
                         ids=lambda x: str(x))
def test_in_rule_philox_noise(shape, first_env, t):
    """u(r, i, p) at counter (first_env + r) S P + i P + p, eps(r, i) at (t + 1) 2^40 + (first_env + r) S + i,
    under noise_key(seed, iteration): the uniforms bit for bit, the normals within philox_ref's criterion."""
    hp = _hp()
    c = hp.cfg(*shape)
    od, S, P, dc = hp.dims(c)
    M, seed, iteration = 5, 2**45 + 3, 6
    key = hp.noise_key(seed, iteration)
    assert key == R.noise_key(seed, iteration) == (seed * 1000003 + iteration) % 2**64
    u, eps = hp.sample_noise(c, M, key, first_env, t)
    cu, ce = R.draw_noise_counters(first_env, M, S, P, t + 1)
    for r, i, p in ((0, 0, 0), (M - 1, S - 1, P - 1), (2, S // 2, 0)):
        assert int(cu.reshape(M, S, P)[r, i, p]) == (first_env + r) * S * P + i * P + p
        assert int(ce[t].reshape(M, S)[r, i]) == (t + 1) * 2**40 + (first_env + r) * S + i
    assert bits(u.ravel(), R.uniform(key, cu))
    z, rad = R.normal64(key, ce[t])
    assert not R.normal_outside(eps.ravel(), z, rad).any()
    if t:  # another step, other normals
        assert (hp.sample_noise(c, M, key, first_env, t - 1)[1] != eps).mean() > 0.9
    # the rule draws these very numbers: the Philox form equals the tape form fed with them
    obs = np.random.default_rng(2).uniform(-1, 1, (M, od)).astype(np.float32)
    rng = np.random.default_rng(3)
    wd = rng.normal(0, 0.3, 32 * dc + 4224 + 66).astype(np.float32)
    wc, ww = (rng.normal(0, 0.3, 32 * 13 + 4224 + 33).astype(np.float32) for _ in range(2))
    a = hp.sample_decide(c, wd, obs, key=key, first_env=first_env)
    b = hp.sample_decide(c, wd, obs, u=u)
    for k in ("a_d", "logp_d", "probs", "feat_d", "closest", "exist"):
        assert bits(a[k], b[k]), k
    x = hp.sample_act(c, wc, ww, obs, a["a_d"], a["closest"], key=key, first_env=first_env, t=t)
    y = hp.sample_act(c, wc, ww, obs, a["a_d"], a["closest"], eps=eps)
    for k in ("actions", "act", "logp", "feat_c"):
        assert bits(x[k], y[k]), k


def test_threaded_rows_equal_serial():
    """tools/hostpolicy.cpp's row loops on 16 threads, on 3 (uneven runs of the 1 000 rows) and on the
    machine's default give the plain loop's bits: every output of the four rules, the status word included
    (scalable 4/2/2: P = 2, absent cars; the Philox forms, whose noise depends on the row's flat index)."""
    import oracle
    hp = _hp()
    g = np.load(os.path.join(ROOT, "tests", "golden", "rollout_scalable_422.npz"))
    c = hp.cfg("scalable", 4, 2, 2)
    M = 1000
    obs = oracle.OracleBatch("scalable", M, 4, 2, 2, seed_base=int(g["seed_base"])).reset()
    key = hp.noise_key(7, 2)
    bad = g["w_cross"].copy()
    bad[-1] = np.nan

    def run():
        d = hp.sample_decide(c, g["w_choice"], obs, key=key, first_env=9)
        a, p = hp.decide(c, g["w_choice"], obs, probs=True)
        noise = dict(key=key, first_env=9, t=3)
        return dict(d=d, s=hp.sample_act(c, g["w_cross"], g["w_wait"], obs, d["a_d"], d["closest"], **noise),
                    nan=hp.sample_act(c, bad, g["w_wait"], obs, d["a_d"], d["closest"], **noise),
                    det=dict(a_d=a, probs=p, actions=hp.act(c, g["w_cross"], g["w_wait"], obs, a)))

    prev = hp.set_threads(1)
    try:
        serial = run()
        assert serial["d"]["status"] == 0 and serial["s"]["status"] == 0 and serial["nan"]["status"] == 2
        assert 0 < serial["d"]["a_d"].sum() < serial["d"]["a_d"].size and (serial["d"]["exist"] == 0).any()
        for n in (16, 3, 0):
            hp.set_threads(n)
            got = run()
            for what, ref in serial.items():
                for k, v in ref.items():
                    assert (got[what][k] == v) if k == "status" else bits(got[what][k], v), (n, what, k)
    finally:
        hp.set_threads(prev)


def test_nan_status():
    """NaN probabilities set status bit 1, a NaN loc bit 2."""
    import oracle
    hp = _hp()
    g = np.load(os.path.join(ROOT, "tests", "golden", "rollout_scalable_422.npz"))
    c = hp.cfg("scalable", 4, 2, 2)
    obs = oracle.OracleBatch("scalable", 6, 4, 2, 2, seed_base=int(g["seed_base"])).reset()
    d = hp.sample_decide(c, g["w_choice"], obs, forced=np.zeros((6, 4, 2), np.int32))
    eps = np.random.default_rng(4).normal(size=(6, 4)).astype(np.float32)
    assert hp.sample_act(c, g["w_cross"], g["w_wait"], obs, d["a_d"], d["closest"], eps=eps)["status"] == 0
    bad = g["w_choice"].copy()
    bad[-1] = np.nan
    assert hp.sample_decide(c, bad, obs, forced=d["a_d"])["status"] == 1
    bad = g["w_cross"].copy()
    bad[-1] = np.nan
    assert hp.sample_act(c, bad, g["w_wait"], obs, d["a_d"], d["closest"], eps=eps)["status"] == 2
