"""The perf-mode noise on the device against tests/philox_ref.py, an independent Philox-4x32-10
that reproduces Random123's known-answer vectors: what the numbers are, not only how they are used.

Uniforms (mhppo_philox_uniform, RolloutGPU.draw_noise's u) are compared bit for bit.  Normals
(mhppo_philox_normal, mhppo_philox_normal_2d, draw_noise's eps) against float64 Box-Muller on the
device's exact float32 inputs, under |device - ref| <= K 2^-23 r with r = sqrt(-2 log u1) the draw's
radius: relative to the radius, not the value, so draws near a zero of the cosine need no floor of
their own.  Expected from ROCm's documented bounds (logf, cosf, sqrtf 1-2 ulp each, an exact doubling,
one rounding for the product): 3-4.  Measured on an MI355X over the 2^20 draws of seed 7:
max |device - ref| / (2^-23 r) = 1.634 (test_normal_1d prints it; at most 1.2 in the other cases);
asserted at K = 4, twice that rounded up to a whole number (philox_ref.K).  The square root is the
correctly rounded one (the compiler's default for sqrtf), which is why the measurement is below the
expectation.  tests/test_noise_host.py shows on these very inputs that every wrong generator it lists
misses this criterion."""
import numpy as np
import pytest
import torch

import philox_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64  # floats behind each output that a launch must leave alone


def launch(name, n, args):
    """Run entry point `name` into a buffer of n floats (plus the guard); float32 numpy [n].
    args(pointer): the call's arguments up to the stream."""
    from mhppo import _lib
    buf = torch.full((n + GUARD,), float("nan"), device="cuda")
    fn = getattr(_lib.lib(), name)
    _lib.check(fn(*args(_lib.ptr(buf)), _lib.stream_ptr()))
    out = buf.cpu().numpy()
    assert np.isnan(out[n:]).all(), "the launch wrote behind its output"
    return out[:n]


def draw_1d(name, seed, off, n):
    return launch(name, n, lambda p: (seed & R.MASK64, off & R.MASK64, p, n))


@pytest.fixture(scope="module")
def ref_1d():
    """(uniform, (normal, radius)) of each 1-D case, computed once."""
    out = {}
    for seed, off, n in R.CASES_1D:
        w = R.words(seed, R.counters(off, n))
        out[seed, off, n] = R.u24(w[..., 0]), R.box_muller64(w[..., 0], w[..., 1])
    return out


def check_normal(dev, z, r, what):
    ratio = np.abs(dev.astype(np.float64) - z) / (2.0 ** -23 * np.where(r > 0, r, 1.0))
    print(f"{what}: max |device - ref| / (2^-23 r) = {ratio[r > 0].max() if (r > 0).any() else 0.0:.3f}")
    assert np.isfinite(dev).all(), what
    assert np.all(dev[r == 0] == 0.0), what  # u1 = 1: exactly zero, of either sign
    bad = R.normal_outside(dev, z, r)
    assert not bad.any(), (what, int(bad.sum()), float(ratio.max()))


@pytest.mark.parametrize("case", R.CASES_1D, ids=lambda c: f"seed{c[0]}-off{c[1]}-n{c[2]}")
def test_uniform_1d(case, ref_1d):
    seed, off, n = case
    u = draw_1d("mhppo_philox_uniform", seed, off, n)
    want = ref_1d[case][0]
    assert np.array_equal(u.view(np.uint32), want.view(np.uint32))
    if (off, n) == (R.CTR_U_ZERO, 1):
        assert u[0] == 0.0
    if (off, n) == (R.CTR_U_MAX, 1):
        assert u[0] == np.float32(1.0 - 2.0 ** -24) and u[0] < 1.0


@pytest.mark.parametrize("case", R.CASES_1D, ids=lambda c: f"seed{c[0]}-off{c[1]}-n{c[2]}")
def test_normal_1d(case, ref_1d):
    seed, off, n = case
    x = draw_1d("mhppo_philox_normal", seed, off, n)
    z, r = ref_1d[case][1]
    check_normal(x, z, r, f"seed {seed} off {off} n {n}")
    if (off, n) == (R.CTR_U_ZERO, 1):  # u1 = 2^-24: the largest radius, finite
        assert r[0] == np.sqrt(48.0 * np.log(2.0)) and np.isfinite(x[0])
    if (off, n) == (R.CTR_U_MAX, 1):  # u1 = 1
        assert r[0] == 0.0 and x[0] == 0.0


@pytest.mark.parametrize("case", R.CASES_2D, ids=lambda c: f"seed{c[0]}-{c[3]}x{c[4]}")
def test_normal_2d(case):
    seed, off, stride, rows, cols = case
    x = launch("mhppo_philox_normal_2d", rows * cols, lambda p: (seed, off, stride, p, rows, cols))
    ctr = R.counters_2d(off, stride, rows, cols)
    if rows > 1:
        assert (ctr[1:].min(1) > ctr[:-1].max(1)).all()  # the rows' counters do not overlap
    z, r = R.normal64(seed, ctr.ravel())
    check_normal(x, z, r, f"2-D seed {seed} {rows} x {cols}")


@pytest.fixture(scope="module")
def rollout():
    from mhppo.env import VecCrosswalk
    from mhppo.rollout import RolloutGPU
    return RolloutGPU(VecCrosswalk("coop", 5, 4, 2, 2, env_id_offset=7))


def noise_ref(ro, key):
    off = int(ro.venv.cfg.env_id_offset)
    cu, ce = R.draw_noise_counters(off, ro.N, ro.S, ro.P, ro.T)
    z, r = R.normal64(key, ce)
    return R.uniform(key, cu), z, r


def test_draw_noise_counters_are_disjoint(rollout):
    """The counters of u and of every step's eps, as draw_noise lays them out for this shape."""
    ro = rollout
    off = int(ro.venv.cfg.env_id_offset)
    assert off == 7 and ro.T >= 2 and ro.u.shape == (ro.N, ro.S, ro.P) and ro.eps.shape == (ro.T, ro.N, ro.S)
    cu, ce = R.draw_noise_counters(off, ro.N, ro.S, ro.P, ro.T)
    sets = [set(int(c) for c in cu)] + [set(int(c) for c in row) for row in ce]
    assert len(sets[0]) == ro.u.numel() and all(len(s) == ro.eps[0].numel() for s in sets[1:])
    assert len(set().union(*sets)) == sum(len(s) for s in sets)
    assert int(ce[1, 0]) >> 32 != int(ce[0, 0]) >> 32  # the steps differ in the counter's high word


@pytest.mark.parametrize("seed,iteration", [(3, 0), (3, 1), (2**45 + 3, 0), (2**63, 5)])
def test_draw_noise(rollout, seed, iteration):
    ro = rollout
    key = R.noise_key(seed, iteration)
    assert key == (seed * 1000003 + iteration) % 2**64
    if seed == 2**45 + 3:
        assert key >> 32
    if seed == 2**63:
        assert seed * 1000003 + iteration >= 2**64  # the key wraps
    u_ref, z, r = noise_ref(ro, key)
    # from the reference side: step 1's normals are not step 0's (the counter's dropped high word)
    assert (z[0] != z[1]).mean() > 0.99
    if (seed, iteration) == (3, 1):  # another iteration, other noise
        u0, z0, _ = noise_ref(ro, R.noise_key(3, 0))
        assert (u_ref != u0).mean() > 0.99 and (z != z0).mean() > 0.99
    ro.u.fill_(float("nan"))
    ro.eps.fill_(float("nan"))
    ro.draw_noise(seed, iteration)
    u = ro.u.cpu().numpy().ravel()
    eps = ro.eps.cpu().numpy().reshape(ro.T, -1)
    assert np.array_equal(u.view(np.uint32), u_ref.view(np.uint32))
    check_normal(eps.ravel(), z.ravel(), r.ravel(), f"draw_noise seed {seed} iteration {iteration}")
