"""GAE(lambda) targets on the host: gae_targets_torch (mhppo.rollout: the executable specification
of mhppo_gae_tm's recurrence and the CPU path) against a brute-force float64 sum, its lam = 1 and
lam = 0 ends, and Algo_PPO's validation of gae_lambda (no GPU needed)."""
import numpy as np
import pytest
import torch

TS = (1, 2, 7, 80)
B = 5


def _case(T, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, B)), rng.standard_normal((T, B)).astype(np.float32)


def _brute(rew, v, gamma, lam):
    """R_t = sum_k (gamma lam)^k delta_{t+k} + V_t, delta_t = r_t + gamma V_{t+1} - V_t, V_T = 0."""
    T = rew.shape[0]
    v = v.astype(np.float64)
    vn = np.concatenate([v[1:], np.zeros((1,) + v.shape[1:])])
    delta = rew + gamma * vn - v
    out = np.empty_like(v)
    for t in range(T):
        out[t] = sum((gamma * lam) ** k * delta[t + k] for k in range(T - t)) + v[t]
    return out


def _ulp_apart(a, b):
    """|a - b| in units of the float32 spacing at the larger magnitude."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (0.99, 1.0), (0.99, 0.0), (1.0, 1.0), (0.9, 0.5)])
def test_recurrence_matches_brute_force(T, gamma, lam):
    from mhppo.rollout import gae_targets_torch
    rew, v = _case(T, 100 + T)
    got = gae_targets_torch(torch.from_numpy(rew), torch.from_numpy(v), gamma, lam)
    assert got.dtype == torch.float32 and got.shape == (T, B)
    want = _brute(rew, v, gamma, lam)
    # the values before the cast against the float64 sum, within 1e-12 relative, element by element
    g64 = gae_targets_torch(torch.from_numpy(rew), torch.from_numpy(v), gamma, lam, out_dtype=torch.float64).numpy()
    rel = np.abs(g64 - want) / np.abs(want)
    print(f"T {T} gamma {gamma} lam {lam}: worst relative error {rel.max():.3g}")
    assert np.all(np.abs(g64 - want) <= 1e-12 * np.abs(want))
    # and bit for bit include/mhppo.h's operation order in numpy, cast once
    r64 = _recurrence64(rew, v, gamma, lam)
    assert np.array_equal(g64, r64)
    assert np.array_equal(got.numpy(), r64.astype(np.float32))


def _recurrence64(rew, v, gamma, lam):
    """include/mhppo.h's operation order in numpy float64, before the cast."""
    T = rew.shape[0]
    out = np.empty(rew.shape)
    nv, A, c = np.zeros(rew.shape[1:]), np.zeros(rew.shape[1:]), gamma * lam
    for t in range(T - 1, -1, -1):
        vt = v[t].astype(np.float64)
        d = (rew[t] + gamma * nv) - vt
        A = d + c * A
        out[t] = A + vt
        nv = vt
    return out


@pytest.mark.parametrize("T", TS)
def test_lambda_one_is_the_reward_to_go(T):
    """lam = 1: R_t = G_t, returns_scan's recurrence G_t = r_t + gamma G_{t+1} in float64 cast to
    float32.  The two float64 values differ by about T 2^-53 (|G| + |V|), so after the cast they
    can differ only at a rounding boundary: at most 1 float32 ulp."""
    from mhppo.rollout import gae_targets_torch
    rew, v = _case(T, 200 + T)
    got = gae_targets_torch(torch.from_numpy(rew), torch.from_numpy(v), 0.99, 1.0).numpy()
    g, G = np.zeros(B), np.empty((T, B))
    for t in range(T - 1, -1, -1):
        g = rew[t] + 0.99 * g
        G[t] = g
    assert np.all(_ulp_apart(got, G.astype(np.float32)) <= 1.0)


@pytest.mark.parametrize("T", TS)
def test_lambda_zero_is_the_one_step_target(T):
    from mhppo.rollout import gae_targets_torch
    rew, v = _case(T, 300 + T)
    got = gae_targets_torch(torch.from_numpy(rew), torch.from_numpy(v), 0.99, 0.0).numpy()
    v64 = v.astype(np.float64)
    vn = np.concatenate([v64[1:], np.zeros((1, B))])
    want = ((rew + 0.99 * vn) - v64) + v64  # the recurrence with c = 0, op for op
    assert np.array_equal(got, want.astype(np.float32))
    assert np.all(_ulp_apart(got, (rew + 0.99 * vn).astype(np.float32)) <= 1.0)


def test_shapes_and_devices():
    from mhppo.rollout import gae_targets_torch
    rew, v = _case(7, 1)
    a = gae_targets_torch(torch.from_numpy(rew), torch.from_numpy(v), 0.99, 0.95)
    b = gae_targets_torch(torch.from_numpy(rew).reshape(7, B, 1), torch.from_numpy(v).reshape(7, B, 1), 0.99, 0.95)
    assert torch.equal(a, b.reshape(7, B))
    with pytest.raises(ValueError):
        gae_targets_torch(torch.from_numpy(rew), torch.from_numpy(v[:3]), 0.99, 0.95)


def test_algo_validates_gae_lambda():
    from mhppo.algo import Algo_PPO
    from mhppo.models import Model_PPO
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gae_lambda"):
            Algo_PPO(Model_PPO, None, gae_lambda=bad)  # raised before the env is touched
    with pytest.raises(ValueError, match="gamma"):
        Algo_PPO(Model_PPO, None, gae_lambda=0.9, gamma=1.5)
    algo = object.__new__(Algo_PPO)
    algo._init_hyperparameters({})
    assert algo.gae_lambda is None
    for ok in (0, 0.0, 0.95, 1, 1.0):
        algo._init_hyperparameters({"gae_lambda": ok})
        assert algo.gae_lambda == float(ok) and isinstance(algo.gae_lambda, float)
