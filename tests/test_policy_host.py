"""The stateless policy's rule (csrc/policy_rule.h, compiled for the CPU: tools/hostpolicy.py) against
the reference's evaluation on its shipped weights (tests/golden/eval_*.npz) and against the C oracle
(oracle.evaluate) on random-init heads: the actions are reproduced from the observation rows alone,
with the decision schedule rebuilt from consecutive rows (a choice is re-decided at an episode's
first row and when the re-decision test of the evaluation fires between two rows)."""
import os
import sys

import numpy as np
import pytest

from test_oracle_eval import CASES, CHOIX_CASES, TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
T = 80
# the fixtures in which a per-row choice differs from the scheduled one somewhere
SCHEDULE_MATTERS = ["coop_212", "naif_111"] + CHOIX_CASES
ORACLE_SHAPES = [("scalable", 4, 2, 2), ("scalable", 8, 3, 4), ("4cars", 4, 1, 2), ("coop", 4, 3, 2),
                 ("stop", 2, 1, 2)]


def _hp():
    import hostpolicy
    return hostpolicy


def scheduled(a_row, obs, variant, P):
    """Per-row decisions a_row [M, S, P] of consecutive rows obs [M, od] (whole 80-row episodes) ->
    the decisions in force at each row: the row's own where a decision is due, else the previous row's."""
    env_off = obs.shape[1] - 9 * P - (4 if variant == "scalable" else 3)
    c = obs[:, env_off + 1]
    due = np.zeros(len(obs), bool)
    due[1:] = (c[1:] != np.float32(P)) if variant == "scalable" else (c[1:] != c[:-1])
    due[::T] = True
    idx = np.maximum.accumulate(np.where(due, np.arange(len(obs)), 0))
    return a_row[idx], due


def _fixture(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", f"eval_{name}.npz"))
    hp = _hp()
    c = hp.cfg(str(g["variant"]), int(g["nb_car"]), int(g["nb_ped"]), int(g["nb_lines"]))
    return g, c


@pytest.mark.parametrize("name", CASES + CHOIX_CASES)
def test_fixture_actions_from_observations(name):
    hp = _hp()
    g, c = _fixture(name)
    K = int(g["episodes"])
    assert all(int(n) == K * T for n in g["n_obs"])
    obs, variant, P = g["obs"], str(g["variant"]), int(g["nb_ped"])
    S = hp.dims(c)[1]
    a_row = hp.decide(c, g["w_choice"], obs)
    a_d, due = scheduled(a_row, obs, variant, P)
    acts = hp.act(c, g["w_cross"], g["w_wait"], obs, a_d)[:, :S]
    rt, at = TOL["acts"]
    err = np.abs(acts - g["acts"].astype(np.float64))
    print(f"{name}: max abs error {err.max():.3g}, {int(due.sum())} of {len(obs)} rows decide")
    np.testing.assert_allclose(acts, g["acts"].astype(np.float64), rtol=rt, atol=at)
    if name in SCHEDULE_MATTERS:  # the schedule is tested: deciding anew at every row misses the bar
        every = hp.act(c, g["w_cross"], g["w_wait"], obs, a_row)[:, :S]
        off = np.abs(every - g["acts"]) > at + rt * np.abs(g["acts"])
        print(f"{name}: {int(off.any(1).sum())} rows off when every row decides")
        assert off.any()


@pytest.mark.parametrize("shape", ORACLE_SHAPES, ids=lambda s: "%s_%d%d%d" % s)
def test_oracle_actions_bit_equal(shape):
    import torch

    import oracle
    from mhppo.models import Model_PPO
    hp = _hp()
    variant, nb_car, nb_ped, nb_lines = shape
    c = hp.cfg(variant, nb_car, nb_ped, nb_lines)
    od, S, P, dc = hp.dims(c)
    torch.manual_seed(7)
    w = [Model_PPO(13, 1, 1).packed().numpy(), Model_PPO(13, 1, 1).packed().numpy(),
         Model_PPO(dc, 2, 2).packed().numpy()]
    res = oracle.evaluate(variant, nb_car, nb_ped, nb_lines, [4242 + e for e in range(8)], 2, *w)
    obs = np.concatenate([r["obs"] for r in res])
    ref = np.concatenate([r["acts"] for r in res])
    assert obs.shape == (8 * 2 * T, od) and ref.dtype == np.float32
    a_d, _ = scheduled(hp.decide(c, w[2], obs), obs, variant, P)
    acts = hp.act(c, w[0], w[1], obs, a_d)[:, :S].astype(np.float32)
    assert np.array_equal(acts.view(np.uint32), ref.view(np.uint32))


def test_dims():
    import oracle
    hp = _hp()
    for name in CASES + CHOIX_CASES:
        g, c = _fixture(name)
        od, S, P, dc = hp.dims(c)
        assert od == g["obs"].shape[1] and S == g["acts"].shape[1] and P == int(g["nb_ped"])
        assert dc == oracle.choice_dim(str(g["variant"]), S)
        assert g["w_choice"].size == 32 * dc + 4224 + 66
    for variant, nb_car, nb_ped, nb_lines in ORACLE_SHAPES:
        od, S, P, dc = hp.dims(hp.cfg(variant, nb_car, nb_ped, nb_lines))
        assert S == (2 * nb_lines if variant == "scalable" else nb_car) and P == nb_ped
        assert dc == oracle.choice_dim(variant, S)
    assert hp.dims(hp.cfg("4cars2", 2, 1, 2))[:3] == (12 * 2 + 3 + 9, 4, 1)  # S = 2 nb_car on the device
    for bad in (hp.cfg(6, 2, 1, 2), hp.cfg("coop", 2, 0, 2), hp.cfg("coop", 17, 1, 2), hp.cfg("scalable", 2, 1, 9)):
        with pytest.raises(ValueError):
            hp.dims(bad)


def test_lights_flat_index_quirk():
    """lights[i] = 2 a_d.flat[i] - 1 over the row's [S, P] block, not a_d[i][0] (P = 2: they differ)."""
    hp = _hp()
    g, c = _fixture("scalable_choix_422")
    od, S, P, dc = hp.dims(c)
    assert P == 2
    obs = g["obs"][:200]
    rng = np.random.default_rng(3)
    for a_d in (hp.decide(c, g["w_choice"], obs), rng.integers(0, 2, (len(obs), S, P)).astype(np.int32)):
        lights = hp.act(c, g["w_cross"], g["w_wait"], obs, a_d)[:, S:]
        assert np.array_equal(lights, 2.0 * a_d.reshape(len(obs), S * P)[:, :S] - 1.0)
    assert not np.array_equal(lights, 2.0 * a_d[:, :, 0] - 1.0)  # the random decisions tell the two apart
