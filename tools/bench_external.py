"""Cost of the external-rollout record pass (mhppo_record_step, csrc/rollout_record.hip) and of the
closed loop built on it (mhppo.external.ExternalRollout).

1. The record launch against what a user of the library without it writes with torch ops on
   SamplingSession's outputs, at M = 65 536 streams:
     identity layout   four copy_ into the [t] slices plus the where-minimum;
     compact layout    four index_select + index_copy_ through rec_of (the present segments and their
                       records listed once per episode, outside the timing) plus the where-minimum.
   HIP events around single calls after warm-up, medians of --reps with min-max, the native launch and
   its yardstick alternating within every repetition.  Target: the native median no larger than the
   yardstick's plus the yardstick's own min-max spread in this run.
   Bytes: 152 per stored segment (13 + 1 + 1 floats and one float64 in, the same out) + 16 per segment of
   ep_min traffic, over the launch's median, as a share of the HBM peak (8.0 TB/s).
2. The closed loop ExternalRollout.collect(VecCrosswalk) against RolloutGPU.collect(graph=False, parts=1)
   at the same shapes, per step (informational), alternating; then one instrumented external episode:
   the medians of its act / env step / record phases.

usage: python tools/bench_external.py [--reps R] [--streams M]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from mhppo import _lib  # noqa: E402
from mhppo.env import VecCrosswalk  # noqa: E402
from mhppo.external import ExternalRollout  # noqa: E402
from mhppo.models import Model_PPO  # noqa: E402
from mhppo.policy import Policy  # noqa: E402
from mhppo.rollout import RolloutGPU  # noqa: E402

HBM_PEAK = 8.0e12
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--streams", type=int, default=65536)
a = ap.parse_args()
L = _lib.lib()
T = 80


def timed_interleaved(fns, reps, warm=3):
    """{name: (median, min, max) ms} of the calls in `fns`, alternated within every repetition."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def record_bytes(n_stored, NS):
    return 152 * n_stored + 16 * NS


def where_min(ep_min, x):
    m = ep_min
    ep_min.copy_(torch.where(m != m, m, torch.where(x != x, x, torch.where(x < m, x, m))))


def bench_record(shape, compact):
    M = a.streams
    torch.manual_seed(7)
    venv = VecCrosswalk(shape[0], M, *shape[1:], seed_base=20)
    S, dc = venv.n_slots, L.mhppo_choice_dim(venv.handle)
    ac, aw = (Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda() for _ in range(2))
    pol = Policy.from_env(venv, ac, aw, Model_PPO(dc, 2, 2).cuda())
    obs = venv.reset()
    d = pol.sample_decide(obs, key=5)
    r = pol.sample_act(obs, d.a_d, d.closest, key=5, t=0)
    _, rew, rl, _ = venv.step(r.actions)
    NS = M * S
    z = lambda shape_, dt: torch.zeros(shape_, dtype=dt, device="cuda")
    t = 1  # a step in the middle of small buffers: T = 3
    recs = [z((3, NS, 13), torch.float32), z((3, NS), torch.float32), z((3, NS), torch.float32), z((3, NS), torch.float64)]
    ep_min = z((M, S), torch.float64)
    rec_buf = z(NS + M + 1, torch.int32) if compact else None
    work = z(max(1, int(L.mhppo_record_work_bytes(M, S)) // 8), torch.float64)
    p, st = _lib.ptr, _lib.stream_ptr()
    _lib.check(L.mhppo_record_begin(p(d.exist), M, S, p(rec_buf), p(ep_min), p(work), st))
    rec_of = rec_buf[:NS] if compact else None
    n_stored = int((rec_of >= 0).sum()) if compact else NS

    def native():
        _lib.check(L.mhppo_record_step(M, S, t, 3, p(r.act), p(r.logp), p(r.feat_c), p(rew), p(rl), p(rec_of),
                                       *[p(x) for x in recs], p(ep_min), st))
    srcs = [r.feat_c.view(NS, 13), r.act.view(NS), r.logp.view(NS), rew.view(NS)]
    if compact:
        seg = torch.nonzero(rec_of >= 0).squeeze(1)
        rk = rec_of[seg].long()

        def yard():
            for dst, x in zip(recs, srcs):
                dst[t].index_copy_(0, rk, x.index_select(0, seg))
            where_min(ep_min, rl)
    else:
        def yard():
            for dst, x in zip(recs, srcs):
                dst[t].copy_(x)
            where_min(ep_min, rl)
    res = timed_interleaved({"yard": yard, "native": native}, a.reps)
    (ym, yl, yh), (nm, nl, nh) = res["yard"], res["native"]
    by = record_bytes(n_stored, NS)
    layout = "compact" if compact else "identity"
    print(f"{shape[0]} {shape[1]}/{shape[2]}/{shape[3]}, {layout} layout: M = {M} streams x {S} slots = {NS} segments, "
          f"{n_stored} stored; {by / 1e6:.1f} MB per launch", flush=True)
    print(f"  yardstick: torch ops ({'index_copy_' if compact else 'copy_'} x 4 + where-minimum)"
          f"   {ym * 1e3:9.1f} us (min {yl * 1e3:.1f} max {yh * 1e3:.1f})", flush=True)
    target = ym + yh - yl
    print(f"  mhppo_record_step                                      {nm * 1e3:9.1f} us (min {nl * 1e3:.1f} max {nh * 1e3:.1f})  "
          f"{nm / ym:.3f} of the yardstick; target <= {target * 1e3:.1f} us: {'met' if nm <= target else 'MISSED'};  "
          f"{by / (nm * 1e-3) / 1e12:.2f} TB/s = {100 * by / (nm * 1e-3) / HBM_PEAK:.1f} % of the HBM peak", flush=True)
    del recs, venv
    torch.cuda.empty_cache()


def bench_loop(shape):
    M = a.streams
    torch.manual_seed(7)
    venv = VecCrosswalk(shape[0], M, *shape[1:], seed_base=20)
    twin = VecCrosswalk(shape[0], M, *shape[1:], seed_base=20)
    ro = RolloutGPU(venv, parts=1)
    ac, aw = (Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda() for _ in range(2))
    ad = Model_PPO(ro.dc, 2, 2).cuda()
    ext = ExternalRollout(Policy.from_env(venv, ac, aw, ad), M, T=T, seed=3)
    res = timed_interleaved({"collector": lambda: ro.collect(ac, aw, ad, seed=3, iteration=1, graph=False, parts=1),
                             "external": lambda: ext.collect(twin, 1)}, a.reps, warm=2)
    (cm, cl, ch), (em, el, eh) = res["collector"], res["external"]
    print(f"{shape[0]} {shape[1]}/{shape[2]}/{shape[3]}: closed loop, M = {M}, T = {T}, per step", flush=True)
    print(f"  RolloutGPU.collect(graph=False, parts=1)   {cm / T * 1e3:9.1f} us (min {cl / T * 1e3:.1f} max {ch / T * 1e3:.1f})",
          flush=True)
    print(f"  ExternalRollout.collect(VecCrosswalk)      {em / T * 1e3:9.1f} us (min {el / T * 1e3:.1f} max {eh / T * 1e3:.1f})  "
          f"{em / cm:.3f} of the collector", flush=True)
    # one instrumented external episode: events between the phases of every step
    ev = lambda: torch.cuda.Event(enable_timing=True)
    marks = []
    with torch.no_grad():
        obs = twin.reset()
        ext.begin(obs, 1)
        for t in range(T):
            e = [ev() for _ in range(4)]
            e[0].record()
            actions = ext.act(obs, t)
            e[1].record()
            obs, rew, rl, _ = twin.step(actions)
            e[2].record()
            ext.record(rew, rl)
            e[3].record()
            marks.append(e)
    torch.cuda.synchronize()
    for name, i in (("act (sample_act)", 0), ("env step (mhppo_env_step)", 1), ("record (mhppo_record_step)", 2)):
        v = [e[i].elapsed_time(e[i + 1]) for e in marks]
        print(f"    {name:30s} {statistics.median(v) * 1e3:9.1f} us per step (median of {T})", flush=True)
    del ro, ext, venv, twin
    torch.cuda.empty_cache()


for shape, compact in ((("coop", 4, 2, 2), False), (("scalable", 8, 2, 4), False), (("scalable", 8, 2, 4), True)):
    bench_record(shape, compact)
for shape in (("coop", 4, 2, 2), ("scalable", 8, 2, 4)):
    bench_loop(shape)
