"""The streaming evaluation statistics on the GPU (mhppo_eval_stats_*, RolloutGPU.evaluate_stats,
Algo_PPO.evaluate_stats): the reference's golden rows through the row kernel against the host
harness (the same source compiled for the CPU), and end to end against get_average over the
trajectories evaluate() returns.  Tolerances: tests/evalstats_common.py."""
import numpy as np
import pytest
import torch

from evalstats_common import FIXTURES, check_dict, load_fixture

pytestmark = pytest.mark.gpu


def _venv(f, n=None):
    from mhppo.env import VecCrosswalk
    return VecCrosswalk(f["variant"], n or f["E"], f["nb_car"], f["nb_ped"], f["nb_lines"], seed_base=f["seed_base"])


def _scan(venv, rows):
    """rows [K, T, E, od] on the device, uploaded step by step through mhppo_eval_stats_row."""
    from mhppo.rollout import EvalStats
    acc = EvalStats(venv)
    acc.begin()
    K, T = rows.shape[:2]
    for k in range(K):
        for t in range(T):
            acc.row(rows[k, t], t, T)
    return acc.fold()


_HOST = {}


def _host(name):
    """The fixture, its rows on the device and the harness's sums (computed once, never modified)."""
    if name not in _HOST:
        import hoststats
        f = load_fixture(name)
        sums, abs_sums = hoststats.stats(f["traj"], f["variant"], f["nb_car"], f["nb_ped"], f["nb_lines"],
                                         want_abs=True)
        _HOST[name] = (f, torch.tensor(f["traj"]).cuda(), sums, abs_sums)
    return _HOST[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_rows_match_harness(name):
    from mhppo.stats import EVS, EVS_COUNTS, EVS_NAMES
    f, rows, ref, ref_abs = _host(name)
    got = _scan(_venv(f), rows).cpu().numpy()
    for j, key in enumerate(EVS_NAMES):
        print(f"{key:12s} got {got[j]!r:26} ref {ref[j]!r:26} sum|term| {ref_abs[j]!r}")
    for key in EVS_COUNTS:
        assert got[EVS[key]] == ref[EVS[key]] and float(got[EVS[key]]).is_integer(), key
    assert got[EVS["EPISODES"]] == f["E"] * f["K"] and got[EVS["ROWS"]] == f["E"] * f["K"] * f["T"]
    for j, key in enumerate(EVS_NAMES):
        if not np.isfinite(ref[j]):  # the same inf, NaN for NaN
            assert (np.isnan(got[j]) and np.isnan(ref[j])) or got[j] == ref[j], key
        else:  # identical terms; only the fold order over the envs differs
            assert abs(got[j] - ref[j]) <= 1e-12 * ref_abs[j], (key, got[j], ref[j])


def test_same_bits_twice_and_on_a_side_stream():
    f, rows, _, _ = _host("scalable_221")
    venv = _venv(f)
    a = _scan(venv, rows)
    b = _scan(venv, rows)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = _scan(venv, rows)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.equal(a.view(torch.int64), c.view(torch.int64))


def test_bad_arguments_rejected():
    from mhppo._lib import MhppoError
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    from mhppo.rollout import EvalStats
    f, rows, _, _ = _host("coop_212")
    acc = EvalStats(_venv(f))
    acc.begin()
    with pytest.raises(MhppoError):
        acc.row(rows[0, 0], 0, 1)  # T < 2
    with pytest.raises(MhppoError):
        acc.row(rows[0, 0], 2, 2)  # t outside [0, T)
    with pytest.raises(ValueError):
        acc.row(rows[0, 0, :2], 0, 80)  # not [N, obs_dim]
    v4 = VecCrosswalk("4cars", 4, 4, 1, 2, seed_base=3)
    with pytest.raises(ValueError) as e:
        EvalStats(v4)
    assert "get_average is defined for" in str(e.value)
    with pytest.raises(ValueError):
        Algo_PPO(Model_PPO, v4, verbose=False).evaluate_stats(1)


def _pair(variant, n, nb_car, nb_ped, nb_lines, seed_base):
    """Two fresh envs with the same seed_base and the same nets."""
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    out = []
    for _ in range(2):
        torch.manual_seed(1234)
        out.append(Algo_PPO(Model_PPO, VecCrosswalk(variant, n, nb_car, nb_ped, nb_lines, seed_base=seed_base),
                            verbose=False))
    for a, b in zip(out[0].nets(), out[1].nets()):
        assert torch.equal(a.flat(), b.flat())
    return out


@pytest.mark.parametrize("variant,n,nb_car,nb_ped,nb_lines,K", [("coop", 8, 2, 1, 2, 3), ("scalable", 70, 4, 2, 2, 2),
                                                                ("naif", 8, 1, 1, 1, 2)],
                         ids=["coop_212", "scalable_422", "naif_111"])
def test_evaluate_stats_matches_get_average(variant, n, nb_car, nb_ped, nb_lines, K):
    from mhppo.stats import get_average
    ref_algo, algo = _pair(variant, n, nb_car, nb_ped, nb_lines, seed_base=77)
    states = ref_algo.evaluate(K)[0]
    # the tolerance was measured against get_average's CPU reductions: the same function, on the host
    ref = get_average(states.cpu(), variant, nb_car, nb_ped, nb_lines)
    assert ref["episodes"] == n * K  # precondition: the equal-width runs are the true episodes
    got = algo.evaluate_stats(K)
    assert set(got) == set(ref)
    check_dict(got, ref)
    a, b = ref_algo.venv.state_dict(), algo.venv.state_dict()
    assert a["cfg"] == b["cfg"] and torch.equal(a["blob"], b["blob"])  # the same env draws, the same final state


def test_memory_is_independent_of_the_history():
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    N, K = 4096, 2
    venv = VecCrosswalk("coop", N, 2, 1, 2, seed_base=5)
    algo = Algo_PPO(Model_PPO, venv, verbose=False)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = algo.evaluate_stats(K)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    one_history = algo.rollout.max_steps * N * venv.obs_dim * 4  # one [T, N, obs_dim] float32
    print(f"peak rise {rise} B, one observation history {one_history} B")
    assert rise < one_history
    assert got["episodes"] == N * K


def test_choix_counts_true_episodes():
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    from mhppo.stats import EVS, EVS_COUNTS
    torch.manual_seed(5)
    algo = Algo_PPO(Model_PPO, VecCrosswalk("scalable", 8, 2, 1, 1, seed_base=9), verbose=False)
    got = algo.evaluate_stats(2, choix=True)
    assert got["episodes"] == 16  # get_average's equal-width runs would merge them into one
    algo.rollout.reset()
    sums = algo.rollout.iterations_stats(algo.actor_net_cross, algo.actor_net_wait, algo.actor_net_choice, 2,
                                         choix=True).cpu().numpy()
    for key in EVS_COUNTS:
        assert np.isfinite(sums[EVS[key]]) and float(sums[EVS[key]]).is_integer(), key
    assert sums[EVS["ROWS"]] == 16 * 80 and sums[EVS["N_PED"]] == 16 and sums[EVS["N_CAR"]] == 32


def test_evaluate_never_reaches_the_new_entry_points(monkeypatch):
    from mhppo import _lib
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    calls = []
    for name in ("eval_stats_bytes", "eval_stats_begin", "eval_stats_row", "eval_stats_fold"):
        real = getattr(_lib, name)
        monkeypatch.setattr(_lib, name, lambda *a, _n=name, _r=real: (calls.append(_n), _r(*a))[1])
    algo = Algo_PPO(Model_PPO, VecCrosswalk("coop", 8, 2, 1, 2, seed_base=11), verbose=False)
    states = algo.evaluate(1)[0]
    algo.get_average(states)
    torch.cuda.synchronize()
    assert calls == []
    algo.evaluate_stats(2)
    assert calls.count("eval_stats_begin") == 1 and calls.count("eval_stats_fold") == 1
    assert calls.count("eval_stats_row") == 2 * 80
