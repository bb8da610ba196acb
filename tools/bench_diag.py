"""Launch time of the PPO diagnostics (mhppo_ppo_diag, csrc/mlp_infer.hip) against one exact
f32-MFMA critic train pass (MHPPO_TRAIN_EXACT_F32) over the same rows, and of the batched forward
(mhppo_mlp_forward): HIP events around each launch after warm-up, in one process.  The default row
count is config 3's continuous batch (65 536 envs x 4 slots x 80 steps / 2 heads = 10 485 760).

--algo also times whole Algo_PPO.train(1) iterations at config 3 (4cars 4/1/2, --envs envs) with
diagnostics off and on (wall clock around a synchronised iteration, after warm-up, alternating):
the opt-in cost per iteration.

usage: python tools/bench_diag.py [--rows M] [--reps R] [--algo] [--envs N] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd")]
import torch  # noqa: E402

from mhppo import ppo  # noqa: E402
from mhppo.models import Model_PPO  # noqa: E402

F32_MFMA_PEAK = 157.3e12


def flops_forward(n_in, n_out):
    return 2 * (32 * n_in + 2048 + 2048 + 32 * n_out)


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


ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10485760)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--json", default="")
ap.add_argument("--algo", action="store_true")
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--iters", type=int, default=8)
a = ap.parse_args()
M = a.rows
torch.manual_seed(0)
actor = Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda()
critic = Model_PPO(13, 1, 0).cuda()
obs = torch.randn(M, 13, device="cuda") * 3
ret = torch.randn(M, device="cuda") * 8 - 20
act = torch.randn(M, device="cuda") - 1
lp = torch.randn(M, device="cuda") * 0.3 - 0.9
head = ppo.Head("c", actor, critic, None, None, obs, act, lp, ret, M)
sums3 = torch.zeros(3, dtype=torch.float64, device="cuda")
res = {"rows": M, "reps": a.reps}
for name, fn, flops in (
        ("diag_13_1", lambda: ppo.k_ppo_diag(head), flops_forward(13, 1) * 2),
        ("critic_exact_f32_pass", lambda: ppo.k_mlp_train(0, critic, obs, ret, m_global=float(M), exact=True, sums=sums3),
         ppo.FLOPS_PER_ROW_CONT),
        ("critic_split_pass", lambda: ppo.k_mlp_train(0, critic, obs, ret, m_global=float(M), sums=sums3),
         ppo.FLOPS_PER_ROW_CONT),
        ("forward_13_1", lambda: actor.forward_rows(obs), flops_forward(13, 1))):
    med, lo, hi = timed(fn, a.reps)
    tf = flops * M / (med * 1e-3)
    res[name] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "flop_per_row": flops, "tflops": tf / 1e12,
                 "frac_f32_mfma_peak": tf / F32_MFMA_PEAK}
    print(f"{name:24s} {med:8.3f} ms (min {lo:.3f} max {hi:.3f})  {tf / 1e12:6.1f} TFLOP/s "
          f"{100 * tf / F32_MFMA_PEAK:5.1f} % of the f32-MFMA peak", flush=True)
res["diag_over_exact_critic"] = res["diag_13_1"]["ms_median"] / res["critic_exact_f32_pass"]["ms_median"]
print(f"diag / exact critic pass: {res['diag_over_exact_critic']:.3f}")
del head, obs, ret, act, lp
torch.cuda.empty_cache()
if a.algo:
    import time

    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    algos = {}
    for on in (False, True):
        venv = VecCrosswalk("4cars", a.envs, 4, 1, 2, seed_base=0)
        torch.manual_seed(0)
        algos[on] = Algo_PPO(Model_PPO, venv, verbose=False, save_curves=False, diagnostics=on)
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
    res["algo"] = {"envs": a.envs, "iters": a.iters, "ms_off": ms[False], "ms_on": ms[True], "ms_off_median": off_ms,
                   "ms_on_median": on_ms, "cost_ms": on_ms - off_ms, "last_entry": algos[True].diagnostics[-1]}
    print(f"Algo_PPO.train(1) at {a.envs} envs: diagnostics off {off_ms:.2f} ms, on {on_ms:.2f} ms "
          f"(+{on_ms - off_ms:.2f} ms per iteration)")
    print("last entry:", json.dumps(algos[True].diagnostics[-1]))
if a.json:
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
