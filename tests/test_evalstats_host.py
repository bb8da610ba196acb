"""The streaming evaluation statistics on the CPU (no GPU needed): csrc/eval_stats_terms.h
compiled for the host (tools/hoststats) over the reference's golden evaluation trajectories, and
mhppo.stats.stats_from_sums, against get_average and the reference's own get_average results
(tests/golden/stats_*.npz).  Tolerances: tests/evalstats_common.py."""
import math
import os

import numpy as np
import pytest
import torch

from evalstats_common import FIXTURES, GOLDEN, check_dict, load_fixture

KEYS_SKIP = {"variant", "nb_car", "nb_ped", "nb_lines", "eval_fixture"}


def _harness_dict(f):
    import hoststats
    from mhppo.stats import stats_from_sums
    sums = hoststats.stats(f["traj"], f["variant"], f["nb_car"], f["nb_ped"], f["nb_lines"])
    return stats_from_sums(sums, f["nb_car"])


@pytest.mark.parametrize("name", FIXTURES)
def test_harness_matches_get_average(name):
    from mhppo.stats import get_average
    f = load_fixture(name)
    ref = get_average(torch.tensor(f["obs"]), f["variant"], f["nb_car"], f["nb_ped"], f["nb_lines"])
    assert ref["episodes"] == f["E"] * f["K"]  # precondition: the equal-width runs are the true episodes
    got = _harness_dict(f)
    assert set(got) == set(ref)
    check_dict(got, ref)


@pytest.mark.parametrize("name", ("scalable_211", "scalable_221"))
def test_harness_matches_reference_golden(name):
    """Against the reference's own function on its own trajectories."""
    s = np.load(os.path.join(GOLDEN, f"stats_{name}.npz"))
    assert str(s["eval_fixture"]) == f"eval_{name}.npz"
    got = _harness_dict(load_fixture(name))
    keys = [k for k in s.files if k not in KEYS_SKIP]
    assert len(keys) >= 20 and set(keys) <= set(got)
    check_dict(got, {k: float(s[k]) for k in keys})


def _sums(**kw):
    from mhppo.stats import EVS, EVS_N
    s = [0.0] * EVS_N
    for k, v in kw.items():
        s[EVS[k]] = float(v)
    return s


def test_stats_from_sums_empty_and_single():
    from mhppo.stats import stats_from_sums
    d = stats_from_sums(_sums(), 1)
    assert d["episodes"] == 0
    for k, v in d.items():  # torch.mean / torch.std / np.mean of an empty list
        if k != "episodes":
            assert math.isnan(v), (k, v)
    assert not any(k.startswith("scenario_") for k in d)
    # one entry per list: the means are the entry, the unbiased stds NaN (torch.std of one element),
    # the population std of the one waiting time 0
    d = stats_from_sums(_sums(ROWS=1, V0=2.0, V0_SQ=4.0, ABSA0=0.5, A0=-0.5, A0_SQ=0.25, ABSVP0=1.0, ABSVP0_SQ=1.0,
                              EPISODES=1, N_PED=1, PEDT=3.0, PEDT_SQ=9.0, WAIT=1.5, WAIT_SQ=2.25, N_CAR=1, CART=6.0,
                              CART_SQ=36.0, FC=-1.0, IC=2.0, N_YSPEED=1, YSPEED=5.0, YSPEED_SQ=25.0, N_YTIME=1,
                              YTIME=0.9, YTIME_SQ=0.81, YIELD=1, N_CS=1, CS=1), 1)
    assert d["mean_speed_car0"] == 2.0 and d["mean_abs_acc_car0"] == 0.5 and d["mean_abs_speed_ped0"] == 1.0
    assert d["mean_pass_time_peds"] == 3.0 and d["mean_pass_time_cars"] == 6.0 and d["mean_waiting_time"] == 1.5
    assert d["interaction_cost"] == 2.0 and d["interaction_cost_max"] == -0.5
    assert d["mean_speed_yielding_cars"] == 5.0 and d["mean_pass_time_yielding_cars"] == 0.9
    for k in ("std_speed_car0", "std_acc_car0", "std_abs_speed_ped0", "std_pass_time_peds", "std_pass_time_cars",
              "std_speed_yielding_cars", "std_pass_time_yielding_cars"):
        assert math.isnan(d[k]), k
    assert d["std_waiting_time"] == 0.0
    assert d["yield_share"] == 1.0 and d["go_share"] == 0.0 and d["could_stop_share"] == 1.0 and d["episodes"] == 1


def test_stats_from_sums_shares_and_scenarios():
    from mhppo.stats import EVS_N, stats_from_sums
    s = _sums(EPISODES=7, N_CAR=14, YIELD=9, GO=5, N_CS=3, CS=1, SC_YY=3, SC_GG=1, SC_GY=2, SC_YG=1)
    d = stats_from_sums(s, 2)
    assert d["yield_share"] == 9 / 7 and d["go_share"] == 5 / 7 and d["could_stop_share"] == 1 / 3
    assert (d["scenario_yield_yield"], d["scenario_go_go"], d["scenario_go_yield"], d["scenario_yield_go"]) == \
        (3 / 7, 1 / 7, 2 / 7, 1 / 7)
    assert type(d["episodes"]) is int and d["episodes"] == 7
    assert not any(k.startswith("scenario_") for k in stats_from_sums(s, 3))
    # a variance that rounds below zero is clamped; non-finite sums pass through as get_average gives them
    d = stats_from_sums(_sums(ROWS=3, V0=0.3, V0_SQ=0.03 - 1e-16, EPISODES=1, N_PED=1, N_CAR=1, FC=-math.inf,
                              IC=math.nan), 1)
    assert d["std_speed_car0"] == 0.0
    assert d["interaction_cost_max"] == -math.inf and math.isnan(d["interaction_cost"])
    with pytest.raises(ValueError):
        stats_from_sums([0.0] * (EVS_N - 1), 1)


def test_rejects_short_episodes_and_4cars():
    import hoststats
    from mhppo.stats import check_variant, split_states
    f = load_fixture("coop_212")
    with pytest.raises(ValueError):
        hoststats.stats(f["traj"][:, :1], f["variant"], f["nb_car"], f["nb_ped"], f["nb_lines"])  # T = 1
    hoststats.stats(f["traj"][:, :2], f["variant"], f["nb_car"], f["nb_ped"], f["nb_lines"])  # T = 2 is the least
    with pytest.raises(ValueError):  # the 4cars layout car|car_follow|env|ped
        hoststats.stats(np.zeros((1, 80, 2, 4 * 12 + 3 + 9), np.float32), "4cars", 4, 1, 2)
    with pytest.raises(ValueError) as a:
        check_variant("4cars")
    with pytest.raises(ValueError) as b:
        split_states(torch.zeros(4, 60), "4cars", 4, 1, 2)
    assert str(a.value) == str(b.value)


def test_two_row_episodes_match_get_average():
    """T = 2, the shortest episode: one pair, l1 and the decision both read at their own rows."""
    import hoststats
    from mhppo.stats import get_average, stats_from_sums
    f = load_fixture("scalable_221")
    traj = np.ascontiguousarray(f["traj"][:, 10:12])  # rows 10, 11 of every episode: [K, 2, E, od]
    obs = np.ascontiguousarray(traj.transpose(2, 0, 1, 3)).reshape(-1, traj.shape[-1])
    ref = get_average(torch.tensor(obs), f["variant"], f["nb_car"], f["nb_ped"], f["nb_lines"])
    assert ref["episodes"] == f["E"] * f["K"]
    check_dict(stats_from_sums(hoststats.stats(traj, f["variant"], f["nb_car"], f["nb_ped"], f["nb_lines"]),
                               f["nb_car"]), ref)
