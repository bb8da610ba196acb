"""Cost of the stateless policy launches (mhppo_policy_decide / mhppo_policy_act, csrc/policy_infer.hip)
against what a user composes today from the parent's entry point on feature rows already in HBM:
  decide  vs one mhppo_mlp_forward of the choice net over [M S P, choice_dim];
  act     vs two mhppo_mlp_forward launches (cross, wait) over [M S P, 13].
HIP events around single launches after warm-up, medians of --reps with min-max, one process.
Observation rows: 64 envs x 70 random-action steps, repeated to M rows; the yardsticks' feature rows
are the same rows' features (tools/hostpolicy.py), repeated alike; a_d from decide.
Target per launch: no longer than its yardstick plus the yardstick's own min-max spread in this run.
The stochastic launches (mhppo_policy_sample_decide / _sample_act) are timed in the same process,
interleaved with the deterministic ones they are measured against:
  sample_decide (feat_d NULL)  vs mhppo_policy_decide with probs;
  sample_decide (with feat_d)  vs the same plus a device copy of M S P choice_dim floats (the bytes it adds);
  sample_act                   vs mhppo_policy_act;
  the in-kernel Philox forms   vs the tape forms plus the mhppo_philox_* launch they replace.
They print their ratio to that yardstick (no target is fixed for them).
FLOP: 2 (32 n_in + 4096 + 32 n_out) per row and forward (13 -> 1: 9 088); act is charged the forwards
its tiles run (a head none of a tile's live, non-override triples uses is skipped).

usage: python tools/bench_policy.py [--reps R]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mh-ppo_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hostpolicy as hp  # noqa: E402
from mhppo import _lib  # noqa: E402
from mhppo.env import VecCrosswalk  # noqa: E402
from mhppo.models import Model_PPO  # noqa: E402
from mhppo.policy import Policy  # noqa: E402

F32_MFMA_PEAK = 157.3e12
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
L = _lib.lib()


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


def timed_interleaved(fns, reps, warm=3):
    """{name: (median, min, max) ms} of the launches in `fns`, alternated within every repetition."""
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


def flop(n_in, n_out):
    return 2 * (32 * n_in + 4096 + 32 * n_out)


def harvest(variant, nb_car, nb_ped, nb_lines, n_envs=64, steps=70, seed=20):
    venv = VecCrosswalk(variant, n_envs, nb_car, nb_ped, nb_lines, seed_base=seed)
    rng = np.random.default_rng(seed)
    rows = [venv.reset()]
    for _ in range(steps - 1):
        act = np.concatenate([rng.uniform(-1.5, 2, (n_envs, venv.n_slots)),
                              rng.choice([-1.0, 1.0], (n_envs, venv.n_slots))], 1)
        rows.append(venv.step(torch.from_numpy(act).cuda())[0])
    return torch.cat(rows)


def report(name, t, yard, fl, ratio_only=False):
    med, lo, hi = t
    if ratio_only:  # a yardstick given as a time in ms: print the ratio, no target
        print(f"  {name:44s} {med * 1e3:9.1f} us (min {lo * 1e3:.1f} max {hi * 1e3:.1f})  {med / yard:.3f} of "
              f"{yard * 1e3:.1f} us", flush=True)
        return
    line = f"  {name:44s} {med * 1e3:9.1f} us (min {lo * 1e3:.1f} max {hi * 1e3:.1f})"
    if fl:
        line += f"  {fl / med / 1e9:6.1f} TFLOP/s = {100 * fl / (med * 1e-3) / F32_MFMA_PEAK:.1f} % of the f32-MFMA peak"
    if yard:
        ym, yl, yh = yard
        line += f"  {med / ym:.3f} of the yardstick; target <= {(ym + yh - yl) * 1e3:.1f} us: {'met' if med <= ym + yh - yl else 'MISSED'}"
    print(line, flush=True)


for shape, M in ((("4cars", 4, 1, 2), 2_621_440), (("scalable", 8, 2, 4), 655_360)):
    c = hp.cfg(*shape)
    od, S, P, dc = hp.dims(c)
    Q = M * S * P
    torch.manual_seed(7)
    ac, aw = (Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda() for _ in range(2))
    ad = Model_PPO(dc, 2, 2).cuda()
    pol = Policy(*shape, ac, aw, ad)
    H = harvest(*shape)
    h_np = H.cpu().numpy()
    reps_h = -(-M // len(H))
    obs = H.repeat(reps_h, 1)[:M].contiguous()
    f13 = torch.from_numpy(hp.features(c, h_np).reshape(-1, 13)).cuda().repeat(reps_h, 1)[:Q].contiguous()
    fd = torch.from_numpy(hp.features_d(c, h_np).reshape(-1, dc)).cuda().repeat(reps_h, 1)[:Q].contiguous()
    a_d = pol.decide(obs)
    # the forwards act's tiles run: per 32-triple tile (P divides 32), each head some live non-override triple uses
    ovr = (f13[:, 7] != 0).view(-1, 32)
    use_w = (a_d.view(-1) > 0).view(-1, 32)
    fwd = int(((~ovr & ~use_w).any(1).sum() + (~ovr & use_w).any(1).sum()).item())
    print(f"{shape[0]} {shape[1]}/{shape[2]}/{shape[3]}: M = {M} rows x {od} floats, {Q} triples, choice_dim {dc}; "
          f"wait share {use_w.float().mean().item():.3f}, override share {ovr.float().mean().item():.3f}, "
          f"act runs {fwd} tile forwards of {2 * (Q // 32)}", flush=True)
    st = _lib.stream_ptr()
    dd, _k0 = ad.mlp_desc()
    dcr, _k1 = ac.mlp_desc()
    dwt, _k2 = aw.mlp_desc()
    probs = torch.empty((Q, 2), dtype=torch.float32, device="cuda")
    out_a = torch.empty_like(a_d)
    mu = torch.empty((2, Q), dtype=torch.float32, device="cuda")
    actions = torch.empty((M, 2 * S), dtype=torch.float64, device="cuda")
    cfgp = ctypes.byref(pol.cfg)

    y_dec = timed(lambda: _lib.check(L.mhppo_mlp_forward(ctypes.byref(dd), _lib.ptr(fd), Q, _lib.ptr(probs), st)), a.reps)
    report(f"yardstick: mlp_forward choice [{Q}, {dc}]", y_dec, None, Q * flop(dc, 2))
    report("mhppo_policy_decide (a_d + probs)",
           timed(lambda: _lib.check(L.mhppo_policy_decide(cfgp, ctypes.byref(dd), _lib.ptr(obs), M, _lib.ptr(out_a),
                                                          _lib.ptr(probs), st)), a.reps), y_dec, Q * flop(dc, 2))
    report("mhppo_policy_decide (a_d only)",
           timed(lambda: _lib.check(L.mhppo_policy_decide(cfgp, ctypes.byref(dd), _lib.ptr(obs), M, _lib.ptr(out_a),
                                                          None, st)), a.reps), y_dec, Q * flop(dc, 2))

    def two_forwards():
        _lib.check(L.mhppo_mlp_forward(ctypes.byref(dcr), _lib.ptr(f13), Q, _lib.ptr(mu[0]), st))
        _lib.check(L.mhppo_mlp_forward(ctypes.byref(dwt), _lib.ptr(f13), Q, _lib.ptr(mu[1]), st))
    y_act = timed(two_forwards, a.reps)
    report(f"yardstick: 2 x mlp_forward [{Q}, 13]", y_act, None, 2 * Q * flop(13, 1))
    for name, dec in (("decided a_d", a_d), ("all cross", torch.zeros_like(a_d)), ("all wait", torch.ones_like(a_d))):
        n_f = fwd if name == "decided a_d" else int((~ovr).any(1).sum().item())
        report(f"mhppo_policy_act ({name})",
               timed(lambda: _lib.check(L.mhppo_policy_act(cfgp, ctypes.byref(dcr), ctypes.byref(dwt), _lib.ptr(obs),
                                                           _lib.ptr(dec), M, _lib.ptr(actions), st)), a.reps),
               y_act, n_f * 32 * flop(13, 1))

    # ---- the stochastic launches, alternated with their yardsticks within every repetition
    Q_, MS = Q, M * S
    u = torch.rand(Q_, device="cuda")
    eps = torch.randn(MS, device="cuda")
    lp_d = torch.empty(Q_, dtype=torch.float32, device="cuda")
    cl = torch.empty(MS, dtype=torch.int32, device="cuda")
    ex = torch.empty(MS, dtype=torch.uint8, device="cuda")
    feat_d = torch.empty((Q_, dc), dtype=torch.float32, device="cuda")
    act = torch.empty(MS, dtype=torch.float32, device="cuda")
    lp = torch.empty(MS, dtype=torch.float32, device="cuda")
    feat_c = torch.empty((MS, 13), dtype=torch.float32, device="cuda")
    key = 3 * 1000003 + 1
    nz_u, nz_e, nz_k = _lib.PolicyNoise(), _lib.PolicyNoise(), _lib.PolicyNoise()
    nz_u.tape, nz_e.tape = u.data_ptr(), eps.data_ptr()
    nz_k.key, nz_k.first_env, nz_k.t = key, 0, 0
    p = _lib.ptr

    def s_decide(nz, fdp):
        return lambda: _lib.check(L.mhppo_policy_sample_decide(cfgp, ctypes.byref(dd), p(obs), M, ctypes.byref(nz),
                                                               p(out_a), p(lp_d), p(probs), fdp, p(cl), p(ex), None, st))

    def s_act(nz, fcp):
        return lambda: _lib.check(L.mhppo_policy_sample_act(cfgp, ctypes.byref(dcr), ctypes.byref(dwt), p(obs), p(a_d),
                                                            p(cl), M, ctypes.byref(nz), p(actions), p(act), p(lp), fcp,
                                                            None, st))
    s_decide(nz_u, None)()  # closest for the act launches
    T = timed_interleaved({
        "y_d": lambda: _lib.check(L.mhppo_policy_decide(cfgp, ctypes.byref(dd), p(obs), M, p(out_a), p(probs), st)),
        "t_d0": s_decide(nz_u, None),
        "y_cp": lambda: feat_d.copy_(fd),
        "t_d1": s_decide(nz_u, p(feat_d)),
        "y_pu": lambda: _lib.check(L.mhppo_philox_uniform(key, 0, p(u), Q_, st)),
        "t_dk": s_decide(nz_k, p(feat_d)),
        "y_a": lambda: _lib.check(L.mhppo_policy_act(cfgp, ctypes.byref(dcr), ctypes.byref(dwt), p(obs), p(a_d), M,
                                                     p(actions), st)),
        "t_a1": s_act(nz_e, p(feat_c)),
        "t_a0": s_act(nz_e, None),
        "y_pn": lambda: _lib.check(L.mhppo_philox_normal(key, 1 << 40, p(eps), MS, st)),
        "t_ak": s_act(nz_k, p(feat_c)),
    }, a.reps)
    y_d, t_d0, y_cp, t_d1, y_pu, t_dk = (T[k] for k in ("y_d", "t_d0", "y_cp", "t_d1", "y_pu", "t_dk"))
    y_a, t_a1, t_a0, y_pn, t_ak = (T[k] for k in ("y_a", "t_a1", "t_a0", "y_pn", "t_ak"))
    report("yardstick: mhppo_policy_decide (a_d + probs)", y_d, None, 0)
    report(f"yardstick: copy of {Q_} x {dc} floats", y_cp, None, 0)
    report("yardstick: mhppo_philox_uniform", y_pu, None, 0)
    report("sample_decide tape, feat_d NULL", t_d0, y_d[0], 0, True)
    report("sample_decide tape, feat_d", t_d1, y_d[0] + y_cp[0], 0, True)
    report("sample_decide Philox, feat_d  (vs tape + philox)", t_dk, t_d1[0] + y_pu[0], 0, True)
    n_s = int(((~use_w).any(1).sum() + use_w.any(1).sum()).item())  # no override: every live triple's head runs
    print(f"  sample_act runs {n_s} tile forwards, mhppo_policy_act {fwd}", flush=True)
    report("yardstick: mhppo_policy_act (decided a_d)", y_a, None, 0)
    report("yardstick: mhppo_philox_normal", y_pn, None, 0)
    report("sample_act tape, feat_c", t_a1, y_a[0], 0, True)
    report("sample_act tape, feat_c NULL", t_a0, y_a[0], 0, True)
    report("sample_act Philox, feat_c  (vs tape + philox)", t_ak, t_a1[0] + y_pn[0], 0, True)
    del u, eps, lp_d, cl, ex, feat_d, act, lp, feat_c
    del obs, f13, fd, a_d, probs, mu, actions
    torch.cuda.empty_cache()
