"""Launch time of the native clip-and-Adam step (mhppo_adam_clip, csrc/adam_clip.hip) against
today's unclipped optimiser step, for the six nets of config 3 (4cars 4/1/2), and the opt-in cost
of Algo_PPO(max_grad_norm=...) per iteration.

Launch: HIP events around single calls after warm-up, medians, one process.  today =
ppo.adam_steps(opts) (one torch._foreach_add_ and one torch._fused_adam_ per distinct lr: 1 + 2
launches, no clipping), native = ppo.adam_steps(opts, max_grad_norm) (one launch: norms, clip,
Adam), torch_clip = clip_grad_norm_ per net + today's step (what the feature would cost on the
torch side).  host = the wall clock of the call itself (no synchronisation inside).

--algo: whole Algo_PPO.train(1) iterations at config 2 (coop 2/1/2, 4096 envs) and config 3
(4cars 4/1/2, 65536 envs) with max_grad_norm off and on (wall clock around a synchronised
iteration, after warm-up, alternating): the opt-in cost per iteration.

usage: python tools/bench_adam.py [--reps R] [--max-norm C] [--algo] [--iters K]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd")]
import torch  # noqa: E402

CONFIGS = {2: ("coop", 2, 1, 2, 4096), 3: ("4cars", 4, 1, 2, 65536)}

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--max-norm", type=float, default=0.5)
ap.add_argument("--algo", action="store_true")
ap.add_argument("--iters", type=int, default=8)
a = ap.parse_args()


def make_algo(cfg, envs=None, **kw):
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    variant, nc, npd, nl, n = CONFIGS[cfg]
    venv = VecCrosswalk(variant, envs or n, nc, npd, nl, seed_base=0)
    torch.manual_seed(0)
    return Algo_PPO(Model_PPO, venv, verbose=False, save_curves=False, **kw)


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms, host = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e6)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ms), min(ms), max(ms), statistics.median(host)


from mhppo import ppo  # noqa: E402

algo = make_algo(3, envs=64)
nets = algo.nets()
opts = [algo.optimizer_actor_cross, algo.optimizer_actor_wait, algo.optimizer_actor_choice,
        algo.optimizer_critic_cross, algo.optimizer_critic_wait, algo.optimizer_critic_choice]
print(f"config 3 nets: {[n.flat().numel() for n in nets]} floats, lr {[o.param_groups[0]['lr'] for o in opts]}")
for n in nets:
    n.grad_flat().normal_(0.0, 0.01)
norms = torch.empty(6, dtype=torch.float64, device="cuda")


def torch_clip():
    for n in nets:
        torch.nn.utils.clip_grad_norm_(n.parameters(), a.max_norm)
    ppo.adam_steps(opts)


# the native path first: it creates the Adam state; today's fast path needs the state to exist
for name, fn in (("native", lambda: ppo.adam_steps(opts, a.max_norm, norms)), ("today", lambda: ppo.adam_steps(opts)),
                 ("torch_clip", torch_clip)):
    ppo.clip_forget()
    for n in nets:  # (clip_grad_norm_ scales the gradients in place: every variant starts from fresh ones)
        n.grad_flat().normal_(0.0, 0.01)
    med, lo, hi, host = timed(fn, a.reps)
    print(f"{name:11s} {med:8.1f} us (min {lo:.1f} max {hi:.1f})   host {host:6.1f} us per call", flush=True)
del algo, nets, opts

if a.algo:
    for cfg in (2, 3):
        algos = {}
        for on in (False, True):
            algos[on] = make_algo(cfg, max_grad_norm=a.max_norm if on else None)
            algos[on].train(3)  # warm-up (allocator, Adam state, plans)
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
        print(f"config {cfg}: Algo_PPO.train(1) max_grad_norm off {off_ms:.2f} ms, {a.max_norm} {on_ms:.2f} ms "
              f"({on_ms - off_ms:+.2f} ms per iteration)   off {[round(x, 2) for x in ms[False]]} "
              f"on {[round(x, 2) for x in ms[True]]}", flush=True)
        del algos
        torch.cuda.empty_cache()
