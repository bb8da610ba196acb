"""Time of ExternalRollout.collect with auto_reset against early_end=True on a simulator that never reports done:
what the per-step re-decision (one uniform launch, one full-M decide launch, the merge) costs when nothing ever
restarts.  Config 3's shape by default (4cars, 65 536 streams x 4 slots, T = 80), the simulator a VecCrosswalk
whose done is replaced by zeros.  The two collectors alternate within every repetition; each collect is timed by
stream events and by the host clock between two device synchronisations.  Prints the median, minimum and maximum
in ms over --reps repetitions and the ratio of the medians.

    python tools/bench_auto_reset.py [--envs 65536] [--reps 10] [--lanes 4]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mh-ppo_amd"))


class NeverDone:
    """A VecCrosswalk whose done is all zeros"""

    def __init__(self, env, M):
        self.env = env
        self.done = torch.zeros(M, dtype=torch.bool, device="cuda")

    def reset(self):
        return self.env.reset()

    def step(self, actions):
        obs, rew, rl, _ = self.env.step(actions)
        return obs, rew, rl, self.done


def line(name, v):
    print(f"  {name:22s} median {statistics.median(v):8.3f} ms  (min {min(v):.3f}, max {max(v):.3f})")


def main():
    from mhppo.env import VecCrosswalk
    from mhppo.external import ExternalRollout
    from mhppo.models import Model_PPO
    from mhppo.policy import Policy
    from mhppo.rollout import RolloutGPU
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lanes", type=int, default=4)
    a = ap.parse_args()
    M = a.envs
    venv = VecCrosswalk("4cars", M, 4, 1, 2, seed_base=0)
    T = RolloutGPU(venv).T
    torch.manual_seed(0)
    ac, aw = (Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda() for _ in range(2))
    ad = Model_PPO(RolloutGPU(venv).dc, 2, 2).cuda()
    pol = Policy.from_env(venv, ac, aw, ad)
    sim = NeverDone(venv, M)
    ext = dict(early_end=ExternalRollout(pol, M, T=T, early_end=True),
               auto_reset=ExternalRollout(pol, M, T=T, auto_reset=a.lanes))

    def timed(e, it):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h0 = time.perf_counter()
        e0.record()
        e.collect(sim, it)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - h0) * 1e3

    for it in range(2):  # warm-up
        for e in ext.values():
            timed(e, it)
    ev, host = {k: [] for k in ext}, {k: [] for k in ext}
    for it in range(a.reps):
        for k, e in ext.items():
            x, y = timed(e, it)
            ev[k].append(x)
            host[k].append(y)
    print(f"4cars, {M} streams x {pol.n_slots} slots, T = {T}, auto_reset = {a.lanes}, {a.reps} repetitions, alternating")
    for k in ext:
        line(k + " (events)", ev[k])
        line(k + " (host)", host[k])
    print(f"  ratio of the medians: events {statistics.median(ev['auto_reset']) / statistics.median(ev['early_end']):.3f}, "
          f"host {statistics.median(host['auto_reset']) / statistics.median(host['early_end']):.3f}")


if __name__ == "__main__":
    main()
