"""Launch time of the GAE(lambda) targets (mhppo_gae_tm, csrc/mlp_gae.hip) against the PPO
diagnostics launch over as many rows (mhppo_ppo_diag kind 1: two forwards and one staging per
tile, no scan), and the opt-in cost of Algo_PPO(gae_lambda=...) per iteration.

Kernel: B records x T steps of 13 inputs, HIP events around each launch after warm-up, medians,
in one process, for three bucket patterns: all one bucket (one critic forwarded per tile),
the bucket plan of a real config-3 collect (4cars 4/1/2; its first B records), alternating buckets
(both critics forwarded on every tile).

--algo: whole Algo_PPO.train(1) iterations at config 2 (coop 2/1/2, 4096 envs) and config 3
(4cars 4/1/2, 65536 envs) with gae_lambda off and on (wall clock around a synchronised iteration,
after warm-up, alternating): the opt-in cost per iteration.

--dp OUT_DIR: the data-parallel rehearsal: one process on 2048 envs and two gloo ranks of 1024
(torch.distributed.run, sharing the GPU) train one iteration with gae_lambda set; the nets must
agree to 1e-5 (the scan is local to a segment: no collective of its own).

usage: python tools/bench_gae.py [--records B] [--steps T] [--reps R] [--algo] [--iters K] [--json PATH]
       python tools/bench_gae.py --dp OUT_DIR"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

F32_MFMA_PEAK = 157.3e12
FLOPS_FORWARD = 2 * (32 * 13 + 2048 + 2048 + 32)  # one 13 -> 32 -> 64 -> 32 -> 1 forward of one row
CONFIGS = {2: ("coop", 2, 1, 2, 4096), 3: ("4cars", 4, 1, 2, 65536)}

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=131072)
ap.add_argument("--steps", type=int, default=80)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--algo", action="store_true")
ap.add_argument("--iters", type=int, default=8)
ap.add_argument("--lam", type=float, default=0.95)
ap.add_argument("--json", default="")
ap.add_argument("--dp", default="", metavar="OUT_DIR")
ap.add_argument("--dp-worker", default="", metavar="OUT", help=argparse.SUPPRESS)
a = ap.parse_args()


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def make_algo(cfg, envs=None, offset=0, **kw):
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    variant, nc, npd, nl, n = CONFIGS[cfg]
    venv = VecCrosswalk(variant, envs or n, nc, npd, nl, seed_base=0, env_id_offset=offset)
    torch.manual_seed(0)
    return Algo_PPO(Model_PPO, venv, verbose=False, save_curves=False, **kw)


if a.dp_worker:  # one rank of the data-parallel rehearsal (tests/dp_worker.py with gae_lambda set)
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo")
    n = 2048 // world
    algo = make_algo(3, envs=n, offset=rank * n, seed=3, gae_lambda=a.lam)
    algo.train(1)
    if rank == 0:
        np.save(a.dp_worker, np.concatenate([net.flat().cpu().numpy() for net in algo.nets()]))
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()
    sys.exit(0)

if a.dp:
    os.makedirs(a.dp, exist_ok=True)
    one, two = os.path.join(a.dp, "gae_dp_one.npy"), os.path.join(a.dp, "gae_dp_two.npy")
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    me = os.path.abspath(__file__)
    subprocess.run([sys.executable, me, "--lam", str(a.lam), "--dp-worker", one], check=True, timeout=240, env=env)
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                    "--master-addr", "127.0.0.1", "--master-port", str(29600 + os.getpid() % 300), me, "--lam",
                    str(a.lam), "--dp-worker", two], check=True, timeout=240, env=env)
    x, y = np.load(one), np.load(two)
    d = float(np.abs(x - y).max())
    print(f"gae_lambda {a.lam}: one process on 2048 envs against two gloo ranks of 1024: {x.size} parameters, "
          f"finite {bool(np.isfinite(x).all() and np.isfinite(y).all())}, max |difference| {d:.3g}")
    sys.exit(0 if np.isfinite(x).all() and d <= 1e-5 else 1)

from mhppo import ppo  # noqa: E402
from mhppo.models import Model_PPO  # noqa: E402
from mhppo.rollout import bucket_plan, gae_targets_tm  # noqa: E402

B, T = a.records, a.steps
M = B * T
torch.manual_seed(0)
actor = Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda()
c0, c1 = Model_PPO(13, 1, 0).cuda(), Model_PPO(13, 1, 0).cuda()
res = {"records": B, "steps": T, "rows": M, "reps": a.reps}

# the plan of a real config-3 collect (its first B records)
algo = make_algo(3)
with torch.no_grad():
    batch = algo.rollout.gpu.collect(algo.actor_net_cross, algo.actor_net_wait, algo.actor_net_choice, seed=0)
plan = bucket_plan(batch)
pos_real, bucket_real = plan["pos"][:B].clone(), plan["bucket"][:B].clone()
n_b1 = int(((pos_real >= 0) & (bucket_real != 0)).sum())
tiles = bucket_real[:B // 32 * 32].reshape(-1, 32)
mixed = int(((tiles != 0).any(1) & (tiles == 0).any(1)).sum())
res["plan"] = {"used": int((pos_real >= 0).sum()), "bucket1": n_b1, "tiles": int(tiles.shape[0]), "mixed_tiles": mixed}
print(f"config-3 plan, first {B} records: {res['plan']}", flush=True)
del algo, batch, plan
torch.cuda.empty_cache()

obs = torch.randn(T, B, 13, device="cuda") * 3
rew = torch.randn(T, B, dtype=torch.float64, device="cuda")
idx = torch.arange(B, device="cuda")
cases = {
    "one_bucket": (idx.clone(), torch.zeros(B, dtype=torch.int8, device="cuda")),
    "config3_plan": (pos_real, bucket_real),
    "alternating": (idx.clone(), (idx & 1).to(torch.int8)),
}
for name, (pos, bucket) in cases.items():
    med, lo, hi = timed(lambda: gae_targets_tm(obs, rew, c0, c1, pos, bucket, 0.99, a.lam), a.reps)
    res["gae_" + name] = {"ms_median": med, "ms_min": lo, "ms_max": hi}
    print(f"gae {name:14s} {med:8.3f} ms (min {lo:.3f} max {hi:.3f})", flush=True)

# the yardstick: the diagnostics launch over the same number of rows, same process
flat = obs.reshape(M, 13)
ret = torch.randn(M, device="cuda") * 8 - 20
act = torch.randn(M, device="cuda") - 1
lp = torch.randn(M, device="cuda") * 0.3 - 0.9
head = ppo.Head("c", actor, c0, None, None, flat, act, lp, ret, M)
med, lo, hi = timed(lambda: ppo.k_ppo_diag(head), a.reps)
tf = 2 * FLOPS_FORWARD * M / (med * 1e-3)
res["diag_13_1"] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "tflops": tf / 1e12}
print(f"diag kind 1        {med:8.3f} ms (min {lo:.3f} max {hi:.3f})  {tf / 1e12:6.1f} TFLOP/s "
      f"{100 * tf / F32_MFMA_PEAK:5.1f} % of the f32-MFMA peak", flush=True)
med, lo, hi = timed(lambda: c0.forward_rows(flat), a.reps)
res["forward_13_1"] = {"ms_median": med, "ms_min": lo, "ms_max": hi}
print(f"forward            {med:8.3f} ms (min {lo:.3f} max {hi:.3f})", flush=True)
for name in cases:
    r = res["gae_" + name]["ms_median"] / res["diag_13_1"]["ms_median"]
    res["gae_" + name]["over_diag"] = r
    print(f"gae {name} / diag: {r:.3f}")
del head, obs, rew, flat, ret, act, lp
torch.cuda.empty_cache()

if a.algo:
    res["algo"] = {}
    for cfg in (2, 3):
        algos = {}
        for on in (False, True):
            algos[on] = make_algo(cfg, gae_lambda=a.lam if on else None)
            algos[on].train(3)  # warm-up (graph capture, allocator, Adam state)
            torch.cuda.synchronize()
        ms = {False: [], True: []}
        for _ in range(a.iters):
            for on in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                algos[on].train(1)
                torch.cuda.synchronize()
                ms[on].append((time.perf_counter() - t0) * 1e3)
        off_ms, on_ms = statistics.median(ms[False]), statistics.median(ms[True])
        res["algo"][f"config{cfg}"] = {"envs": CONFIGS[cfg][4], "iters": a.iters, "ms_off": ms[False], "ms_on": ms[True],
                                       "ms_off_median": off_ms, "ms_on_median": on_ms, "cost_ms": on_ms - off_ms}
        print(f"config {cfg}: Algo_PPO.train(1) gae_lambda off {off_ms:.2f} ms, {a.lam} {on_ms:.2f} ms "
              f"({on_ms - off_ms:+.2f} ms per iteration)", flush=True)
        del algos
        torch.cuda.empty_cache()
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
