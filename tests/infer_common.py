"""Shared pieces of tests/test_infer_host.py and tests/test_infer_gpu.py: the host harness
(tools/libhostfwd.so: the device source compiled for the CPU), seeded nets and batches, and the
diagnostics' per-row terms written directly in numpy float64."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_INS = (5, 13, 27, 54, 64)
KINDS = (0, 1, 2)
MEAN, STD = -1.0, 3.0
# csrc/ppo_math.h LN_0_8 / LN_1_2: the doubles d at which the float64 exp(d) reaches 0.8 / leaves 1.2
LN_0_8, LN_1_2 = float.fromhex("-0x1.c8ff7c79a9a22p-3"), float.fromhex("0x1.7565011e49678p-3")
MVN_L = np.float32(math.sqrt(0.5))


def hostfwd():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import hostfwd as hf
    return hf


def make_net(kind, n_in, seed, device="cpu"):
    from mhppo.models import Model_PPO
    torch.manual_seed(seed)
    net = Model_PPO(n_in, 2 if kind == 2 else 1, kind, mean=MEAN, std=STD)
    return net.to(device) if device != "cpu" else net


def packed_np(net):
    return net.packed().cpu().numpy().copy()


def randn(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def perturbed(W, sigma, seed):
    return (W.astype(np.float64) + sigma * np.random.default_rng(seed).standard_normal(W.shape)).astype(np.float32)


def ref_forward64(kind, W, X, n_in):
    """The head in float64 torch ops from the packed float32 weights."""
    W = torch.from_numpy(np.asarray(W, np.float64))
    x = torch.from_numpy(np.asarray(X, np.float64))
    n_out = 2 if kind == 2 else 1
    off = 0
    h = x
    for i, (o, k) in enumerate(((32, n_in), (64, 32), (32, 64), (n_out, 32))):
        w = W[off:off + o * k].reshape(o, k)
        off += o * k
        b = W[off:off + o]
        off += o
        h = torch.nn.functional.linear(h, w, b)
        if i < 3:
            h = torch.relu(h)
    assert off == W.numel()
    if kind == 2:
        return torch.softmax(h, -1).numpy()
    if kind == 1:
        return (torch.tanh(h[:, 0]) * STD + MEAN).numpy()
    return h[:, 0].numpy()


def diag_case(akind, n_in, M, sigma, seed):
    """A diagnostics batch: X ~ N(0, 1), act and logp_old drawn from / computed with the
    unperturbed actor (through the host harness), ret = V_0 + noise, then both nets perturbed by
    sigma * randn.  Returns a dict of numpy arrays (W*0: before, W*: after the perturbation)."""
    hf = hostfwd()
    Wa0 = packed_np(make_net(akind, n_in, seed))
    Wc0 = packed_np(make_net(0, n_in, seed + 1))
    X = randn((M, n_in), seed + 2)
    rng = np.random.default_rng(seed + 3)
    V0 = hf.forward(0, Wc0, X)
    ret = (V0 + 0.5 * rng.standard_normal(M).astype(np.float32)).astype(np.float32)
    if akind == 1:
        mu0 = hf.forward(1, Wa0, X, MEAN, STD)
        act = (mu0 + MVN_L * rng.standard_normal(M).astype(np.float32)).astype(np.float32)
        logp_old = hf.mvn_logp(act, mu0)
    else:
        p = hf.forward(2, Wa0, X)
        act = (rng.random(M).astype(np.float32) >= p[:, 0] / (p[:, 0] + p[:, 1])).astype(np.int32)
        _, _, logp_old = hf.diag_rows(2, Wa0, Wc0, X, act, np.zeros(M, np.float32), ret)
    return dict(akind=akind, n_in=n_in, M=M, X=X, act=act, logp_old=logp_old, ret=ret, Wa0=Wa0, Wc0=Wc0,
                Wa=perturbed(Wa0, sigma, seed + 4), Wc=perturbed(Wc0, sigma, seed + 5))


def host_terms(c, Wa=None, Wc=None):
    hf = hostfwd()
    return hf.diag_rows(c["akind"], c["Wa"] if Wa is None else Wa, c["Wc"] if Wc is None else Wc, c["X"], c["act"],
                        c["logp_old"], c["ret"], MEAN, STD)


def numpy_terms(c, logp_new, probs=None, V=None):
    """[M, 10] per-row terms in numpy float64 from the heads' outputs."""
    d = logp_new.astype(np.float64) - c["logp_old"].astype(np.float64)
    t = np.zeros((c["M"], 10))
    t[:, 0] = d
    t[:, 1] = np.expm1(d) - d
    t[:, 2] = (d < LN_0_8) | (d > LN_1_2)
    t[:, 3] = np.exp(d)
    if probs is not None:
        eps = np.float32(1.1920928955078125e-07)
        s = probs[:, 0] + probs[:, 1]
        n = np.clip(probs / s[:, None], eps, np.float32(1.0) - eps).astype(np.float64)
        t[:, 4] = -(n[:, 0] * np.log(n[:, 0]) + n[:, 1] * np.log(n[:, 1]))
    g, v = c["ret"].astype(np.float64), V.astype(np.float64)
    t[:, 5], t[:, 6], t[:, 7], t[:, 8], t[:, 9] = g - v, (g - v) ** 2, g, g * g, v
    return t
