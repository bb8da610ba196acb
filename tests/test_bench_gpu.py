"""bench.py's command line: a plain run stops at the headline figure, `--steps` sets the number
of timed iterations, `--dump-outputs DIR` writes the last timed iteration's nets and reward-curve
entries, `--full` adds the measurements that take runs of their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ("actor_net_cross", "actor_net_wait", "actor_net_choice",
        "critic_net_cross", "critic_net_wait", "critic_net_choice")
FULL_ONLY = ("roofline", "roofline_env", "rollout_step_us", "cpu_baseline")


def _bench(tmp_path, *args):
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", "1024",
                          "--warmup", "1"] + list(args), check=True, timeout=300, env=env, cwd=tmp_path,
                         capture_output=True, text=True).stdout
    return json.loads([x for x in out.splitlines() if x.startswith("{")][-1])


def test_plain_run_and_dump_outputs(tmp_path):
    d = tmp_path / "out"
    nets = str(tmp_path / "nets.npy")
    line = _bench(tmp_path, "--steps", "3", "--dump-outputs", str(d), "--save-nets", nets)
    assert line["steps"] == 3 and len(line["iter_ms"]) == 3
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0
    np.testing.assert_allclose(line["value"], 1024 * 80 / (line["ms_per_step"] * 1e-3), rtol=1e-9)
    assert not [k for k in FULL_ONLY if k in line]
    assert sorted(os.listdir(d)) == sorted([n + ".npy" for n in NETS] + ["reward_curves.npy",
                                                                        "scenario_balance.npy"])
    flat = []
    for n in NETS:
        w = np.load(d / (n + ".npy"))
        assert w.dtype == np.float32 and w.ndim == 1 and w.size > 0 and np.isfinite(w).all()
        flat.append(w)
    # the dump is the timed path's last step: the nets as they stand after it (--save-nets)
    assert np.array_equal(np.concatenate(flat), np.load(nets))
    rc, bal = np.load(d / "reward_curves.npy"), np.load(d / "scenario_balance.npy")
    assert rc.dtype == np.float64 and rc.shape == (3,) and bal.dtype == np.float64 and bal.shape == (2,)
    assert np.isfinite(rc[2]) and (bal >= 0).all() and bal.sum() > 0
    assert np.isfinite(rc[:2][bal > 0]).all()


def test_full_adds_the_other_measurements(tmp_path):
    line = _bench(tmp_path, "--steps", "1", "--full", "--cpu-sample-envs", "64")
    assert line["steps"] == 1 and len(line["iter_ms"]) == 1 and line["ms_per_step"] > 0
    for k in FULL_ONLY:
        assert k in line, k
    assert line["roofline"]["launches"] > 0 and line["roofline_env"]["kernel_ms"] > 0
    assert line["cpu_baseline"]["value"] > 0
