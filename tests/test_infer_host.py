"""The batched head forward and the PPO diagnostics on the CPU (no GPU): the host harness
(tools/hostfwd.cpp: mlp_forward and the host+device finishes / per-row terms of
csrc/mlp_infer_terms.h, the source the GPU kernels run) against torch float64 and numpy, the pure
diag_stats, and the binding of the new entry points."""
import math

import numpy as np
import pytest

import infer_common as ic

M = 257


@pytest.mark.parametrize("n_in", ic.N_INS)
@pytest.mark.parametrize("kind", ic.KINDS)
def test_hf_forward_vs_torch_float64(kind, n_in):
    """tests/test_policy_torch_gpu.py's tolerances for the fmaf-chain forward against another
    summation order: outputs within 1e-5 (1 + |ref|), probabilities within 1e-4 relative."""
    hf = ic.hostfwd()
    W = ic.packed_np(ic.make_net(kind, n_in, 100 + 10 * kind + n_in))
    X = ic.randn((M, n_in), 7 + n_in)
    out = hf.forward(kind, W, X, ic.MEAN, ic.STD)
    ref = ic.ref_forward64(kind, W, X, n_in)
    assert out.shape == ref.shape and out.dtype == np.float32
    if kind == 2:
        rel = np.abs(out - ref) / ref
        print(f"kind 2 n_in {n_in}: max relative difference {rel.max():.3g}")
        assert rel.max() <= 1e-4
    else:
        err = np.abs(out - ref) / (1.0 + np.abs(ref))
        print(f"kind {kind} n_in {n_in}: max scaled difference {err.max():.3g}")
        assert err.max() <= 1e-5


@pytest.mark.parametrize("akind,n_in,sigma", [(1, 13, 0.05), (2, 27, 0.1), (2, 54, 0.1), (1, 5, 0.05)])
def test_hf_diag_rows_vs_numpy(akind, n_in, sigma):
    """The harness's per-row terms summed against the same quantities written in numpy float64
    from hf_forward's outputs: only the summation order differs (1e-12 sum |term|)."""
    hf = ic.hostfwd()
    c = ic.diag_case(akind, n_in, M, sigma, 300 + n_in)
    d, terms, lp = ic.host_terms(c)
    assert terms.shape == (M, hf.DIAG_N) and hf.DIAG_N == 10
    V = hf.forward(0, c["Wc"], c["X"])
    if akind == 1:
        mu = hf.forward(1, c["Wa"], c["X"], ic.MEAN, ic.STD)
        # mvn_logp in float32, operation by operation (numpy float32 scalars round every step)
        x = (c["act"] - mu) * np.float32(float.fromhex("0x1.6a09e6p+0"))
        lp_np = (np.float32(-0.5) * (np.float32(float.fromhex("0x1.d67f1cp+0")) + x * x)
                 - np.float32(float.fromhex("-0x1.62e432p-2")))
        assert lp_np.dtype == np.float32 and np.array_equal(lp_np, lp)
        ref = ic.numpy_terms(c, lp_np, None, V)
    else:
        p = hf.forward(2, c["Wa"], c["X"])
        eps = np.float32(1.1920928955078125e-07)
        n = np.clip(p / (p[:, 0] + p[:, 1])[:, None], eps, np.float32(1.0) - eps)
        pa = n[np.arange(M), c["act"]]
        # logf is the C library's (<= 1 ulp from the exact value): the harness's log-probability is
        # checked against the float64 log and then used as is
        exact = np.log(pa.astype(np.float64))
        assert np.all(np.abs(lp.astype(np.float64) - exact) <= np.spacing(np.abs(lp)).astype(np.float64))
        ref = ic.numpy_terms(c, lp, p, V)
    assert np.array_equal(d, ref[:, 0])
    assert np.array_equal(terms[:, 2], ref[:, 2])
    got, want, scale = terms.sum(0), ref.sum(0), np.abs(ref).sum(0)
    for k in range(10):
        print(f"term {k}: {got[k]!r} vs {want[k]!r} (sum |term| {scale[k]:.3g})")
        assert abs(got[k] - want[k]) <= 1e-12 * scale[k]
    assert 0 < terms[:, 2].sum() < M  # the perturbation moves some ratios out of [0.8, 1.2]
    if akind == 1:
        assert np.all(terms[:, 4] == 0.0)
    else:
        assert np.all((terms[:, 4] > 0.0) & (terms[:, 4] <= math.log(2.0)))


def test_hf_diag_rows_unperturbed_is_exactly_zero():
    """With the weights that produced logp_old, d is 0 in every row: K3 0, ratio 1, no clip."""
    for akind, n_in in ((1, 13), (2, 27)):
        c = ic.diag_case(akind, n_in, 64, 0.0, 900 + n_in)
        d, terms, _ = ic.host_terms(c, c["Wa0"], c["Wc0"])
        assert np.all(d == 0.0) and np.all(terms[:, :3] == 0.0) and np.all(terms[:, 3] == 1.0)


def test_diag_stats_hand_made():
    from mhppo import ppo
    s = [0.0] * ppo.DIAG_N
    s[ppo.DIAG_DSUM], s[ppo.DIAG_K3], s[ppo.DIAG_CLIP], s[ppo.DIAG_RATIO], s[ppo.DIAG_ENT] = -2.0, 0.5, 3.0, 11.0, 4.0
    # G = (1, 2, 3, 4, ...), G - V = +-0.5 alternating over 10 rows
    G = np.arange(1.0, 11.0)
    E = np.where(np.arange(10) % 2 == 0, 0.5, -0.5)
    s[ppo.DIAG_E], s[ppo.DIAG_E2], s[ppo.DIAG_G], s[ppo.DIAG_G2] = E.sum(), (E * E).sum(), G.sum(), (G * G).sum()
    s[ppo.DIAG_V] = (G - E).sum()
    st = ppo.diag_stats(s, 10)
    assert st["approx_kl"] == 0.05 and st["kl_k1"] == 0.2 and st["clip_frac"] == 0.3
    assert st["ratio_mean"] == 1.1 and st["entropy"] == 0.4 and st["value_mse"] == 0.25
    assert st["explained_var"] == pytest.approx(1.0 - 0.25 / G.var(), rel=1e-14)
    assert "entropy" not in ppo.diag_stats(s, 10, entropy=False)
    # a perfect critic, a useless one
    s2 = list(s)
    s2[ppo.DIAG_E] = s2[ppo.DIAG_E2] = 0.0
    assert ppo.diag_stats(s2, 10)["explained_var"] == 1.0
    # constant returns: no variance to explain
    s3 = list(s)
    s3[ppo.DIAG_G], s3[ppo.DIAG_G2] = 20.0, 40.0
    assert math.isnan(ppo.diag_stats(s3, 10)["explained_var"])
    # one row
    s4 = [0.25, 0.03, 1.0, 1.28, 0.6, -0.5, 0.25, 3.0, 9.0, 3.5]
    st = ppo.diag_stats(s4, 1)
    assert st["approx_kl"] == 0.03 and st["kl_k1"] == -0.25 and st["clip_frac"] == 1.0 and st["ratio_mean"] == 1.28
    assert st["entropy"] == 0.6 and st["value_mse"] == 0.25 and math.isnan(st["explained_var"])
    # tensors are accepted as well as lists
    import torch
    assert ppo.diag_stats(torch.tensor(s4, dtype=torch.float64), 1)["approx_kl"] == 0.03


def test_binding_declares_the_new_entry_points():
    from mhppo import _lib
    names = set(_lib.declared_symbols())
    assert {"mhppo_mlp_forward", "mhppo_ppo_diag_work_bytes", "mhppo_ppo_diag"} <= names
    L = _lib.lib()
    assert L.mhppo_ppo_diag_work_bytes(0) >= 8
    assert L.mhppo_ppo_diag_work_bytes(4099) >= 8 * 10
    assert L.mhppo_ppo_diag_work_bytes(10_485_760) % 8 == 0

