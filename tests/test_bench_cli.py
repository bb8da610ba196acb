"""bench.py without a GPU: the options' defaults and the layout of `--dump-outputs`."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Net:
    def __init__(self, k):
        self.w = torch.arange(k, k + 5, dtype=torch.float32)

    def flat(self):
        return self.w


class _Algo:
    """The surface dump_outputs reads: nets() in Algo_PPO's order and curves()."""

    def __init__(self, balance):
        self._nets = [_Net(10 * i) for i in range(6)]
        self.balance = balance

    def nets(self):
        return self._nets

    def curves(self):
        return [0.5, -1.5], [0.25], [3.0, 4.0], [[7, 2], self.balance]


def test_defaults_are_a_plain_run(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_layout(tmp_path):
    d = tmp_path / "a" / "b"  # created if missing
    algo = _Algo([3, 0])      # last iteration: no wait rows -> that curve entry is NaN, not a stale one
    bench.dump_outputs(str(d), algo)
    names = ("actor_net_cross", "actor_net_wait", "actor_net_choice",
             "critic_net_cross", "critic_net_wait", "critic_net_choice")
    assert sorted(os.listdir(d)) == sorted([n + ".npy" for n in names] + ["reward_curves.npy",
                                                                         "scenario_balance.npy"])
    for n, net in zip(names, algo.nets()):
        w = np.load(d / (n + ".npy"))
        assert w.dtype == np.float32 and np.array_equal(w, net.w.numpy())
    rc, bal = np.load(d / "reward_curves.npy"), np.load(d / "scenario_balance.npy")
    assert rc.dtype == np.float64 and bal.dtype == np.float64
    assert rc[0] == -1.5 and np.isnan(rc[1]) and rc[2] == 4.0
    assert np.array_equal(bal, [3.0, 0.0])
