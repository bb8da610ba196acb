"""The KL early stop's two measurements (the section on target_kl), each alternating its two
arms in one process after a warm-up, timed with events on the stream.

  python tools/bench_target_kl.py kernel [--rows 1048576] [--reps 30]
      mhppo_ppo_kl against mhppo_ppo_diag on the same rows: a 13-input continuous head and the
      36-input choice head (call = the kernel and its fold).  Medians, and the spread between repeats.
  python tools/bench_target_kl.py iter [--envs 65536] [--steps 12] [--warmup 3]
      one training iteration of the benchmark's config (4cars 4/1/2) with max_grad_norm=inf alone against
      max_grad_norm=inf, target_kl=inf: the same Adam path, so the difference is the nine KL launches per
      head.  Two algos built as bench.py builds its own, one iteration of each in turn.
Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd")]
import torch  # noqa: E402


def spread(xs):
    xs = sorted(xs)
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4),
            "p10_ms": round(xs[len(xs) // 10], 4), "p90_ms": round(xs[(9 * len(xs)) // 10], 4), "n": len(xs)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def kernel(args):
    from mhppo import ppo
    from mhppo.models import Model_PPO
    out = {"mode": "kernel", "rows": args.rows, "reps": args.reps}
    for name, kind, n_in in (("cont13", "c", 13), ("choice36", "d", 36)):
        torch.manual_seed(1)
        actor = Model_PPO(n_in, 2 if kind == "d" else 1, 2 if kind == "d" else 1, mean=-1.0, std=3.0).cuda()
        critic = Model_PPO(n_in, 1, 0).cuda()
        M = args.rows
        obs = torch.randn(M, n_in, device="cuda")
        act = torch.randn(M, device="cuda") if kind == "c" else torch.randint(0, 2, (M,), device="cuda", dtype=torch.int32)
        logp = -torch.rand(M, device="cuda")
        head = ppo.Head(kind, actor, critic, None, None, obs, act, logp, torch.randn(M, device="cuda"), M)
        for _ in range(5):
            ppo.k_ppo_kl(head), ppo.k_ppo_diag(head)
        torch.cuda.synchronize()
        ev = {"kl": [], "diag": []}
        for _ in range(args.reps):
            ev["kl"].append(timed(lambda: ppo.k_ppo_kl(head)))
            ev["diag"].append(timed(lambda: ppo.k_ppo_diag(head)))
        torch.cuda.synchronize()
        out[name] = {k: spread([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}
    return out


def iteration(args):
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    arms = {}
    for name, kw in (("clip_inf", {"max_grad_norm": math.inf}),
                     ("clip_inf_target_kl_inf", {"max_grad_norm": math.inf, "target_kl": math.inf})):
        venv = VecCrosswalk("4cars", args.envs, 4, 1, 2, seed_base=0, device="cuda:0")
        torch.manual_seed(0)
        arms[name] = Algo_PPO(Model_PPO, venv, verbose=False, seed=0, save_curves=False, **kw)
    for _ in range(args.warmup):
        for algo in arms.values():
            algo.train(1)
    torch.cuda.synchronize()
    ev = {k: [] for k in arms}
    for _ in range(args.steps):
        for k, algo in arms.items():
            ev[k].append(timed(lambda: algo.train(1)))
    torch.cuda.synchronize()
    out = {"mode": "iter", "envs": args.envs, "steps": args.steps, "warmup": args.warmup}
    out.update({k: spread([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()})
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["kernel", "iter"])
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    print(json.dumps(kernel(a) if a.mode == "kernel" else iteration(a)), flush=True)
