"""Shared by tests/test_adam_clip_host.py, tests/test_adam_clip_gpu.py and tools/adam_clip_tolerance.py:
the product's net shapes, the accuracy case of the clip-and-Adam contract (include/mhppo.h
mhppo_adam_clip) against float64 torch, and the recorded yardstick."""
import numpy as np
import torch


def model_segs(n_in, n_out):
    """The eight parameter tensors W1 b1 .. W4 b4 of a Model_PPO, as element counts in flat order."""
    return [32 * n_in, 32, 64 * 32, 64, 32 * 64, 32, 32 * n_out, n_out]


# the six nets of the scalable 8-slot product (cross / wait actors and critics 13 -> 1, the choice
# actor 54 -> 2 and critic 54 -> 1), actors first as Algo_PPO orders them: 4 673 .. 6 018 floats
PRODUCT_NETS = [(13, 1), (13, 1), (54, 2), (13, 1), (13, 1), (54, 1)]
PRODUCT_LRS = [3e-4, 3e-4, 3e-4, 1e-3, 1e-3, 1e-3]
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8

# tools/adam_clip_tolerance.py -> profiles/adam_clip/tolerance.txt: the worst parameter error
# |d| / max(1, |ref|) of today's float32 path (float32 clip_grad_norm_ + float32 torch.optim.Adam)
# against the float64 reference on accuracy_case(); the contract may be at most 4x as far.
YARDSTICK_WORST = 3.795e-08
ACC_MAX_NORM = 1.0
ACC_STEPS = 3
# gradient scales per net: norms of about 0.3 .. 4 around ACC_MAX_NORM (sigma sqrt(n))
ACC_NORMS = [0.3, 0.6, 0.9, 1.5, 2.5, 4.0]


def accuracy_case(seed=0):
    """(params, grads): per net a list of float32 parameter tensors (normal * 0.1) and, per step, a
    list of float32 gradient tensors whose norm is about ACC_NORMS[net] (x 0.7 .. 1.3 by step)."""
    rng = np.random.default_rng(seed)
    params, grads = [], [[] for _ in range(ACC_STEPS)]
    for k, (n_in, n_out) in enumerate(PRODUCT_NETS):
        segs = model_segs(n_in, n_out)
        n = sum(segs)
        params.append([torch.from_numpy((0.1 * rng.standard_normal(s)).astype(np.float32)) for s in segs])
        for step in range(ACC_STEPS):
            sigma = ACC_NORMS[k] * (0.7 + 0.3 * step) / np.sqrt(n)
            grads[step].append([torch.from_numpy((sigma * rng.standard_normal(s)).astype(np.float32)) for s in segs])
    return params, grads


def torch_path(params, grads, dtype):
    """clip_grad_norm_ + torch.optim.Adam (one optimiser per net) in `dtype` on CPU copies.
    Returns (final parameters per net as float64 flat vectors, norms [step][net])."""
    nets = [[torch.nn.Parameter(p.to(dtype).clone()) for p in ps] for ps in params]
    opts = [torch.optim.Adam(ps, lr, betas=(BETA1, BETA2), eps=EPS) for ps, lr in zip(nets, PRODUCT_LRS)]
    norms = []
    for step_grads in grads:
        row = []
        for ps, gs, o in zip(nets, step_grads, opts):
            for p, g in zip(ps, gs):
                p.grad = g.to(dtype).clone()
            row.append(float(torch.nn.utils.clip_grad_norm_(ps, ACC_MAX_NORM)))
            o.step()
        norms.append(row)
    return [torch.cat([p.detach().reshape(-1) for p in ps]).double() for ps in nets], norms


def spec_path(params, grads):
    """The contract (mhppo.ppo.adam_clip_torch) on float32 CPU copies, from zero moments."""
    from mhppo import ppo
    nets = [[p.clone() for p in ps] for ps in params]
    state = [[(torch.zeros_like(p), torch.zeros_like(p), torch.zeros((), dtype=torch.float32)) for p in ps]
             for ps in nets]
    norms = []
    for t, step_grads in enumerate(grads, 1):
        row = []
        for ps, gs, st, lr in zip(nets, step_grads, state, PRODUCT_LRS):
            segs = [(p, g, m, v, s) for p, g, (m, v, s) in zip(ps, gs, st)]
            row.append(ppo.adam_clip_torch(segs, t, lr, BETA1, BETA2, EPS, ACC_MAX_NORM))
        norms.append(row)
    return [torch.cat([p.reshape(-1) for p in ps]).double() for ps in nets], norms


def worst_error(got, ref):
    return max(float(((g - r).abs() / r.abs().clamp(min=1.0)).max()) for g, r in zip(got, ref))
