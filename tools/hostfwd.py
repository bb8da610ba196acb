"""ctypes wrapper of tools/libhostfwd.so: the batched head forward and the PPO diagnostics'
per-row terms compiled for the CPU from the device source (csrc/rollout_dev.h mlp_forward,
csrc/mlp_infer_terms.h), and the heads' per-row arithmetic of csrc/ppo_heads.h.  numpy in, numpy out."""
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
                     ("hf_philox_normal", [U64, U64, I64, P]),
                     ("hf_finish_cont", [ctypes.c_int, P, F, F, I64, P, P]), ("hf_softmax_pair", [ctypes.c_int, P, I64, P]),
                     ("hf_cat_normalise", [P, I64, P, P]), ("hf_cat_clamp", [P, I64, P]),
                     ("hf_adv_moments", [P, ctypes.c_double, P]), ("hf_adv_normalised", [P, F, F, I64, P]),
                     ("hf_cont_logp_x", [P, P, I64, P, P]),
                     ("hf_choice_term", [P, P, P, P, ctypes.c_double, I64, P, P]),
                     ("hf_cont_row", [ctypes.c_int, P, F, F, P, P, P, ctypes.c_double, I64, P, P]),
                     ("hf_choice_row", [P, P, P, P, ctypes.c_double, ctypes.c_int, I64, P, P])):
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


# ---- csrc/ppo_heads.h (update=True: the LibmUpdate flavour with the host's libm; False: LibmRollout)
def finish_cont(z, mean, std, update):
    """(tanh(z) * std + mean, tanh(z))"""
    z = _f32(z)
    out, t = np.zeros(z.shape, np.float32), np.zeros(z.shape, np.float32)
    L.hf_finish_cont(int(update), _p(z), float(mean), float(std), z.size, _p(out), _p(t))
    return out, t


def softmax_pair(z, update):
    z = _f32(z)
    p = np.zeros(z.shape, np.float32)
    L.hf_softmax_pair(int(update), _p(z), z.shape[0], _p(p))
    return p


def cat_normalise(p):
    """(pn [M, 2], p0 + p1 [M])"""
    p = _f32(p)
    pn, sp = np.zeros(p.shape, np.float32), np.zeros(p.shape[0], np.float32)
    L.hf_cat_normalise(_p(p), p.shape[0], _p(pn), _p(sp))
    return pn, sp


def cat_clamp(pn):
    pn = _f32(pn)
    out = np.zeros(pn.shape, np.float32)
    L.hf_cat_clamp(_p(pn), pn.size, _p(out))
    return out


def adv_moments(stats, m_global):
    """(meanf, stdf) as float32 scalars from stats = (sum A, sum A^2)"""
    stats, out = _f64(stats), np.zeros(2, np.float32)
    L.hf_adv_moments(_p(stats), float(m_global), _p(out))
    return out[0], out[1]


def adv_normalised(a, meanf, stdf):
    a = _f32(a)
    out = np.zeros(a.shape, np.float32)
    L.hf_adv_normalised(_p(a), float(meanf), float(stdf), a.size, _p(out))
    return out


def cont_logp_x(act, mu):
    """(logp, x) of the update's float64-difference form"""
    act, mu = _f32(act), _f32(mu)
    lp, x = np.zeros(act.shape, np.float32), np.zeros(act.shape, np.float32)
    L.hf_cont_logp_x(_p(act), _p(mu), act.size, _p(lp), _p(x))
    return lp, x


def choice_term(pn, old, A, w, inv_m2):
    """(fk, dL/dpn_k) of one action per element"""
    pn, old, A, w = _f32(pn), _f64(old), _f64(A), _f64(w)
    fk, dlp = np.zeros(pn.shape, np.float64), np.zeros(pn.shape, np.float64)
    L.hf_choice_term(_p(pn), _p(old), _p(A), _p(w), float(inv_m2), pn.size, _p(fk), _p(dlp))
    return fk, dlp


def cont_row(y, mean, std, act, lp_old, A, inv_m, fd):
    """The continuous actor's row (f [M] float64, dL/dy [M] float32); fd: the split-precision form."""
    y, act, lp_old, A = _f32(y), _f32(act), _f32(lp_old), _f32(A)
    f, dy = np.zeros(y.shape, np.float64), np.zeros(y.shape, np.float32)
    L.hf_cont_row(int(fd), _p(y), float(mean), float(std), _p(act), _p(lp_old), _p(A), float(inv_m), y.size, _p(f),
                  _p(dy))
    return f, dy


def choice_row(y, lp_old, A, w, inv_m2, skip_zero):
    """The choice actor's row from y [M, 2] with weights w [M, 2]: (f [M] float64, dL/dy [M, 2] float32)."""
    y, lp_old, A, w = _f32(y), _f32(lp_old), _f32(A), _f64(w)
    f, dy = np.zeros(y.shape[0], np.float64), np.zeros(y.shape, np.float32)
    L.hf_choice_row(_p(y), _p(lp_old), _p(A), _p(w), float(inv_m2), int(skip_zero), y.shape[0], _p(f), _p(dy))
    return f, dy
