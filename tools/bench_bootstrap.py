"""Time of the truncation bootstrap (mhppo_boot_values and the bootstrapped scans, mhppo.rollout) on one rollout
batch: config 3's shape by default (4cars, 65 536 envs x 4 slots, T = 80), the early-end tests' schedule (stream r
ends after 1 + (7 r) mod T steps, every fifth never) with alternating truncated flags (trunc[r] = r & 1), the
streams still running cut at T as truncations, the tail rows given.

  1. mhppo_boot_values alone against what a caller composes from the entry points that were there before it: a
     torch gather of the successor rows (index tensors prepared outside the timed region), two mhppo_mlp_forward
     calls and a where.  HIP events; native and yardstick alternate within every repetition; the results are
     compared bit for bit first.
  2. bucket_segments on the ragged batch: as it is, with boot (reward-to-go), with GAE, with boot and GAE.  Host
     clock between two device synchronisations (the bucketing has one host read of its own inside).
Prints the median, minimum and maximum in ms over --reps repetitions.

    python tools/bench_bootstrap.py [--envs 65536] [--reps 20]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mh-ppo_amd"))


def line(name, v, extra=""):
    print(f"  {name:14s} median {statistics.median(v):8.3f} ms  (min {min(v):.3f}, max {max(v):.3f}){extra}")


def main():
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    from mhppo.rollout import RolloutBatch, RolloutGPU, boot_values, bucket_plan, bucket_segments
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    N = a.envs
    venv = VecCrosswalk("4cars", N, 4, 1, 2, seed_base=0)
    ro = RolloutGPU(venv)
    T, S = ro.T, ro.S
    NS = N * S
    torch.manual_seed(0)
    ac, aw = (Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda() for _ in range(2))
    ad = Model_PPO(ro.dc, 2, 2).cuda()
    c0, c1 = Model_PPO(13, 1, 0).cuda(), Model_PPO(13, 1, 0).cuda()
    batch = ro.collect(ac, aw, ad, seed=0, iteration=0)
    r = torch.arange(N, device="cuda")
    lens = torch.where(r % 5 == 4, torch.zeros_like(r), 1 + (7 * r) % T).to(torch.int32)
    trunc = (r & 1).to(torch.uint8)
    tail = batch.obs_c_tm[T - 1].clone()  # any feature rows will do for the time
    rag = RolloutBatch(**batch.__dict__, len=lens, steps=T)
    boot = RolloutBatch(**batch.__dict__, len=lens, steps=T, trunc=trunc, feat_tail=tail, cut_truncates=True)

    # ---- 1. mhppo_boot_values against the composition
    plan = bucket_plan(boot)
    pos, bucket = plan["pos"], plan["bucket"]
    obs = batch.obs_c_tm.reshape(T, NS, 13)
    ln = lens.long().repeat_interleave(S)
    ended = ln >= 1
    L = torch.where(ended, ln, torch.full_like(ln, T))
    rec = L < T
    sel = (pos >= 0) & torch.where(ended, trunc.repeat_interleave(S) != 0, torch.ones_like(ended))
    Lc, col, b1 = torch.where(rec, L, torch.zeros_like(L)), torch.arange(NS, device="cuda"), bucket != 0
    tail2, zero = tail.reshape(NS, 13), torch.zeros((), dtype=torch.float32, device="cuda")

    def native():
        return boot_values(c0, c1, pos, bucket, None, lens, trunc, N, S, T, True, obs, tail)

    def yardstick():
        rows = torch.where(rec[:, None], obs[Lc, col], tail2)
        return torch.where(sel, torch.where(b1, c1.forward_rows(rows), c0.forward_rows(rows)), zero)

    same = torch.equal(native().view(torch.int32), yardstick().view(torch.int32))
    print(f"4cars, {N} envs x {S} slots, T = {T}, {a.reps} repetitions, alternating")
    print(f"boot_values: {int(sel.sum())} of {NS} segments bootstrapped ({int((sel & rec).sum())} from a record row); "
          f"native == composition bit for bit: {same}")
    if not same:
        sys.exit("mhppo_boot_values differs from the composition")

    def timed_ev(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(3):
        native(), yardstick()
    torch.cuda.synchronize()
    ms = dict(native=[], yardstick=[])
    for _ in range(a.reps):
        ms["native"].append(timed_ev(native))
        ms["yardstick"].append(timed_ev(yardstick))
    for name, v in ms.items():
        line(name, v)
    spread = max(ms["yardstick"]) - min(ms["yardstick"])
    target = statistics.median(ms["yardstick"]) + spread
    print(f"  target: native median <= yardstick median + its min-max spread = {target:.3f} ms: "
          f"{'met' if statistics.median(ms['native']) <= target else 'MISSED'}")

    # ---- 2. the bucketing
    gae = (c0, c1, 0.99, 0.95)
    variants = {"ragged": (rag, {}), "ragged+boot": (boot, dict(boot=(c0, c1))), "ragged+gae": (rag, dict(gae=gae)),
                "ragged+boot+gae": (boot, dict(gae=gae, boot=(c0, c1)))}

    def timed(b, kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bucket_segments(b, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for b, kw in variants.values():  # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            timed(b, kw)
    ms = {name: [] for name in variants}
    for _ in range(a.reps):
        for name, (b, kw) in variants.items():
            ms[name].append(timed(b, kw))
    print("bucket_segments:")
    med = {name: statistics.median(v) for name, v in ms.items()}
    for name, v in ms.items():
        base = "ragged+gae" if name == "ragged+boot+gae" else "ragged"
        line(name, v, "" if name == base else f"  {med[name] - med[base]:+.3f} ms against {base}")


if __name__ == "__main__":
    main()
