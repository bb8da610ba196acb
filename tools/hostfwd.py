"""ctypes wrapper of tools/libhostfwd.so: the batched head forward and the PPO diagnostics'
per-row terms compiled for the CPU from the device source (csrc/rollout_dev.h mlp_forward,
csrc/mlp_infer_terms.h).  numpy in, numpy out."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
L = ctypes.CDLL(os.path.join(HERE, "libhostfwd.so"))
P = ctypes.c_void_p
F = ctypes.c_float
L.hf_forward.restype = ctypes.c_int
L.hf_forward.argtypes = [ctypes.c_int, ctypes.c_int, P, F, F, P, ctypes.c_int64, P]
L.hf_diag_rows.restype = ctypes.c_int
L.hf_diag_rows.argtypes = [ctypes.c_int, ctypes.c_int, P, F, F, P, P, ctypes.c_int64, P, P, P, P, P, P]
L.hf_mvn_logp.restype = None
L.hf_mvn_logp.argtypes = [P, P, ctypes.c_int64, P]
I64, U64 = ctypes.c_int64, ctypes.c_uint64
for _name, _args in (("hf_mvn_sample", [P, P, I64, P]), ("hf_surr_and_grad", [P, P, I64, P, P]),
                     ("hf_surr_and_grad_fd", [P, P, P, I64, P, P]), ("hf_t_minimum", [P, P, I64, P]),
                     ("hf_philox_words", [U64, U64, I64, P]), ("hf_philox_uniform", [U64, U64, I64, P]),
                     ("hf_philox_normal", [U64, U64, I64, P])):
    getattr(L, _name).restype = None
    getattr(L, _name).argtypes = _args
L.hf_diag_n.restype = ctypes.c_int
DIAG_N = L.hf_diag_n()


def _p(a):
    return a.ctypes.data_as(P)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def forward(kind, W, X, mean=0.0, std=1.0):
    """Head of `kind` with packed weights W over X [M, n_in]: [M] (kinds 0, 1) or [M, 2] (kind 2)."""
    W, X = _f32(W), _f32(X)
    M, n_in = X.shape
    out = np.zeros((M, 2) if kind == 2 else (M,), np.float32)
    if L.hf_forward(kind, n_in, _p(W), float(mean), float(std), _p(X), M, _p(out)) != 0:
        raise ValueError(f"hf_forward: kind {kind} / n_in {n_in} not supported")
    return out


def diag_rows(akind, Wa, Wc, X, act, logp_old, ret, mean=0.0, std=1.0):
    """Per-row d [M], terms [M, DIAG_N] and logp_new [M] of the diagnostics (actor of kind 1 / 2)."""
    Wa, Wc, X = _f32(Wa), _f32(Wc), _f32(X)
    M, n_in = X.shape
    act = np.ascontiguousarray(act, np.int32 if akind == 2 else np.float32)
    logp_old, ret = _f32(logp_old), _f32(ret)
    d = np.zeros(M, np.float64)
    terms = np.zeros((M, DIAG_N), np.float64)
    lp = np.zeros(M, np.float32)
    if L.hf_diag_rows(akind, n_in, _p(Wa), float(mean), float(std), _p(Wc), _p(X), M, _p(act), _p(logp_old), _p(ret),
                      _p(d), _p(terms), _p(lp)) != 0:
        raise ValueError(f"hf_diag_rows: kind {akind} / n_in {n_in} not supported")
    return d, terms, lp


def mvn_logp(act, mu):
    act, mu = _f32(act), _f32(mu)
    out = np.zeros(act.shape, np.float32)
    L.hf_mvn_logp(_p(act), _p(mu), act.size, _p(out))
    return out


def _f64(a):
    return np.ascontiguousarray(a, np.float64)


def mvn_sample(loc, eps):
    """ppo_math.h mvn_sample, element by element (float32)."""
    loc, eps = _f32(loc), _f32(eps)
    out = np.zeros(loc.shape, np.float32)
    L.hf_mvn_sample(_p(loc), _p(eps), loc.size, _p(out))
    return out


def surr_and_grad(r, A):
    """ppo_math.h surr_and_grad (float64): the surrogate and df/dr."""
    r, A = _f64(r), _f64(A)
    f, g = np.zeros(r.shape, np.float64), np.zeros(r.shape, np.float64)
    L.hf_surr_and_grad(_p(r), _p(A), r.size, _p(f), _p(g))
    return f, g


def surr_and_grad_fd(r, d, A):
    """ppo_math.h surr_and_grad_fd: float32 ratio r and advantage A, float64 d = lp - lp_old."""
    r, d, A = _f32(r), _f64(d), _f32(A)
    f, g = np.zeros(r.shape, np.float32), np.zeros(r.shape, np.float32)
    L.hf_surr_and_grad_fd(_p(r), _p(d), _p(A), r.size, _p(f), _p(g))
    return f, g


def t_minimum(a, b):
    a, b = _f32(a), _f32(b)
    out = np.zeros(a.shape, np.float32)
    L.hf_t_minimum(_p(a), _p(b), a.size, _p(out))
    return out


_M64 = (1 << 64) - 1


def philox_words(seed, ctr0, n):
    """The four Philox words of draws ctr0 .. ctr0 + n - 1 (mod 2^64) under `seed`: uint32 [n, 4]."""
    out = np.zeros((n, 4), np.uint32)
    L.hf_philox_words(int(seed) & _M64, int(ctr0) & _M64, n, _p(out))
    return out


def philox_uniform(seed, ctr0, n):
    out = np.zeros(n, np.float32)
    L.hf_philox_uniform(int(seed) & _M64, int(ctr0) & _M64, n, _p(out))
    return out


def philox_normal(seed, ctr0, n):
    """Box-Muller with the host's libm (the device's logf / cosf / sqrtf differ in the last bits)."""
    out = np.zeros(n, np.float32)
    L.hf_philox_normal(int(seed) & _M64, int(ctr0) & _M64, n, _p(out))
    return out
