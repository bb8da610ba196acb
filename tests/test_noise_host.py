"""The perf-mode noise on the CPU (no GPU): philox(), the draw helpers of csrc/ppo_math.h compiled
for the host (tools/hostfwd.cpp hf_philox_*), against tests/philox_ref.py, a Philox-4x32-10 written
from the algorithm's definition that reproduces Random123's known-answer vectors; the two edge
draws of seed 7; the power of tests/test_noise_gpu.py's comparison on its own inputs; and the
argument handling of the C entry points (the paths that return before any HIP call).

Two mistakes are invisible to the normal's tolerance.  u1 without its `+ 1` moves u1 by 2^-24,
which changes a typical draw by less than the criterion allows: it is caught only at the edge
counter whose 24-bit word is 0 (log 0: an infinite draw where the reference has the largest finite
radius).  2 pi as a double constant instead of float32 changes the angle by at most a float32
rounding, below the tolerance and harmless: that one is not covered."""
import ctypes

import numpy as np
import pytest

import infer_common as ic
import philox_ref as R

CTRS = (0, 2**32 - 1, 2**32, 2**40 + 5, 81 * 2**40, 2**64 - 1)
SEEDS = (0, 7, 2**32, 2**63 + 1)


def test_known_answer_vectors():
    for c, k, out in R.KAT:
        got = R.philox4x32(c, k)
        assert got.shape == (4,) and [int(x) for x in got] == list(out)
    # arrays of counters give the same words as one counter at a time
    c = [np.array([v[0][j] for v in R.KAT], np.uint64) for j in range(4)]
    assert all(int(R.philox4x32(c, R.KAT[2][1])[2, j]) == R.KAT[2][2][j] for j in range(4))


def test_reference_conventions():
    """The project's counter block and key on top of philox4x32, and the counter taken mod 2^64."""
    seed, ctr = 2**63 + 1, 81 * 2**40 + 3
    w = R.words(seed, ctr)
    want = R.philox4x32((ctr & R.MASK32, ctr >> 32, 0x6D687070, 0), (seed & R.MASK32, seed >> 32))
    assert np.array_equal(w, want)
    assert np.array_equal(R.words(seed, ctr + 2**64), w) and np.array_equal(R.words(seed + 2**64, ctr), w)
    assert np.array_equal(R.words(seed, R.counters(2**64 - 2, 4))[3], R.words(seed, 1))
    assert [int(c) for c in R.counters(2**64 - 2, 4)] == [2**64 - 2, 2**64 - 1, 0, 1]


@pytest.mark.parametrize("seed", SEEDS)
def test_hf_philox_words(seed):
    hf = ic.hostfwd()
    for ctr in CTRS:
        got = hf.philox_words(seed, ctr, 3)  # ctr, ctr + 1, ctr + 2 (mod 2^64)
        want = R.words(seed, R.counters(ctr, 3))
        assert got.dtype == np.uint32 and np.array_equal(got.astype(np.uint64), want), (seed, ctr)


def test_hf_philox_uniform_straddles_2_32():
    hf = ic.hostfwd()
    for seed in (7, 2**63 + 1):
        ctr0 = 2**32 - 2048
        got = hf.philox_uniform(seed, ctr0, 4096)
        want = R.uniform(seed, R.counters(ctr0, 4096))
        assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert len(np.unique(got)) > 4000  # the high word of the counter matters


def test_hf_philox_normal():
    """ppo_math.h's Box-Muller with the host's libm against the float64 reference under the GPU
    test's criterion (glibc's logf / cosf / sqrtf are within 1 ulp, so the asserted k holds here
    as well)."""
    hf = ic.hostfwd()
    for seed, ctr0 in ((7, 0), (2**63 + 1, 2**40 - 1000)):
        got = hf.philox_normal(seed, ctr0, 1 << 16)
        z, r = R.normal64(seed, R.counters(ctr0, 1 << 16))
        ratio = np.abs(got - z) / (2.0 ** -23 * r)
        print(f"seed {seed}: host max |draw - ref| / (2^-23 r) = {ratio.max():.3f}")
        assert not R.normal_outside(got, z, r).any()


def test_edge_draws():
    hf = ic.hostfwd()
    # 24-bit word 0: the uniform is exactly 0, the normal has u1 = 2^-24, the largest radius
    w = R.words(7, R.CTR_U_ZERO)
    assert int(w[0]) >> 8 == 0
    assert R.uniform(7, R.CTR_U_ZERO) == 0.0 and hf.philox_uniform(7, R.CTR_U_ZERO, 1)[0] == 0.0
    z, r = R.normal64(7, R.CTR_U_ZERO)
    assert r == np.sqrt(48.0 * np.log(2.0)) and abs(r - 5.768) < 1e-3 and np.isfinite(z)
    got = hf.philox_normal(7, R.CTR_U_ZERO, 1)
    assert np.isfinite(got[0]) and not R.normal_outside(got, z, r).any()
    # 24-bit word 0xFFFFFF: the largest uniform; the normal has u1 = 1, so it is exactly zero
    w = R.words(7, R.CTR_U_MAX)
    assert int(w[0]) >> 8 == 0xFFFFFF
    top = np.float32(1.0 - 2.0 ** -24)
    assert R.uniform(7, R.CTR_U_MAX) == top and hf.philox_uniform(7, R.CTR_U_MAX, 1)[0] == top and top < 1.0
    z, r = R.normal64(7, R.CTR_U_MAX)
    assert r == 0.0 and z == 0.0
    assert hf.philox_normal(7, R.CTR_U_MAX, 1)[0] == 0.0


# ---------------------------------------------------------------- power of the GPU comparison
# name -> (changes the uniforms, changes the normals, which draws it changes)
def _all(seed, ctr):
    return np.ones(ctr.shape, bool)


VARIANTS = {
    "counter high word dropped": (True, True, lambda seed, ctr: (ctr >> np.uint64(32)) != 0),
    "seed high word dropped": (True, True, lambda seed, ctr: np.full(ctr.shape, (seed & R.MASK64) >> 32 != 0)),
    "9 rounds": (True, True, _all),
    "key increments swapped": (True, True, _all),
    "words 0 and 1 swapped": (True, True, _all),
    "u2 from word 0": (False, True, _all),
    "sin for cos": (False, True, _all),
}


def variant_draws(name, seed, ctr):
    """(uniform, normal) of a wrong generator, from philox_ref's own pieces."""
    seed = int(seed) & R.MASK64
    lo, hi, key, kw = ctr & np.uint64(R.MASK32), ctr >> np.uint64(32), [seed & R.MASK32, seed >> 32], {}
    if name == "counter high word dropped":
        hi = np.zeros_like(hi)
    elif name == "seed high word dropped":
        key[1] = 0
    elif name == "9 rounds":
        kw["rounds"] = 9
    elif name == "key increments swapped":
        kw["bumps"] = (R.W1, R.W0)
    w = R.philox4x32((lo, hi, R.TAG, 0), key, **kw)
    w0, w1 = w[..., 0], w[..., 1]
    if name == "words 0 and 1 swapped":
        w0, w1 = w1, w0
    if name == "u2 from word 0":
        w1 = w0
    return R.u24(w0), box_muller(w0, w1, np.sin if name == "sin for cos" else np.cos)


def box_muller(w0, w1, trig):
    return R.box_muller64(w0, w1, trig)[0]


def gpu_inputs():
    """(seed, counters, has a uniform case) of every launch of tests/test_noise_gpu.py's kernel cases."""
    for seed, off, n in R.CASES_1D:
        yield seed, R.counters(off, n), True
    for seed, off, stride, rows, cols in R.CASES_2D:
        yield seed, R.counters_2d(off, stride, rows, cols).ravel(), False


@pytest.fixture(scope="module")
def reference_draws():
    return [(seed, ctr, uni, R.uniform(seed, ctr), R.normal64(seed, ctr)) for seed, ctr, uni in gpu_inputs()]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_gpu_comparison_has_power(name, reference_draws):
    """Each wrong generator differs from the reference on the inputs the GPU test uses, beyond the
    GPU test's criterion (bits for the uniforms, k 2^-23 r at the asserted k for the normals), in
    more than 99 % of the draws it changes at all: two unrelated 24-bit words coincide once in
    2^24 draws, and two unrelated normals lie within k 2^-23 r ~ 1e-6 r of each other about as
    rarely."""
    in_u, in_n, touched = VARIANTS[name]
    nu = du = nn = dn = 0
    for seed, ctr, uni, u_ref, (z_ref, r_ref) in reference_draws:
        t = touched(seed, ctr)
        if not t.any():
            continue
        u, z = variant_draws(name, seed, ctr)
        if uni:
            nu += int(t.sum())
            du += int((u.view(np.uint32) != u_ref.view(np.uint32))[t].sum())
        nn += int(t.sum())
        dn += int(R.normal_outside(z, z_ref, r_ref)[t].sum())
        if in_u:  # a draw the variant does not touch is the reference's
            assert np.array_equal(u[~t], u_ref[~t])
        assert not R.normal_outside(z, z_ref, r_ref)[~t].any()
    print(f"{name}: uniforms {du} of {nu} touched draws differ ({100.0 * du / max(nu, 1):.4f} %), "
          f"normals {dn} of {nn} beyond k = {R.K} ({100.0 * dn / max(nn, 1):.4f} %)")
    assert nn >= 8 and nu >= 8, "the GPU test's inputs do not reach this mistake"
    if in_u:
        assert du > 0.99 * nu
    else:
        assert du == 0
    assert in_n and dn > 0.99 * nn


def test_draw_noise_layout_has_power():
    """RolloutGPU.draw_noise's counters for 5 envs of 4 slots and 2 pedestrians from env id 7 over 80
    steps (tests/test_noise_gpu.py takes its shape from the object): with the counter's high word
    dropped every step's normals would be step 0's.  The reference's own steps differ in more than
    99 % of positions."""
    N, S, P, T, off = 5, 4, 2, 80, 7
    cu, ce = R.draw_noise_counters(off, N, S, P, T)
    assert cu.shape == (N * S * P,) and ce.shape == (T, N * S)
    assert int(cu[0]) == off * S * P and int(ce[2, 3]) == 3 * 2**40 + off * S + 3
    key = R.noise_key(3, 0)
    z = R.normal64(key, ce)[0]
    assert (z[0] != z[1]).mean() > 0.99
    dropped = variant_draws("counter high word dropped", key, ce)[1]
    assert np.array_equal(dropped[0], dropped[1]) and np.array_equal(dropped[0], dropped[T - 1])


# ---------------------------------------------------------------- C-ABI argument handling
EINVAL, OK = -1, 0


def test_noise_entry_points_check_their_arguments():
    """Bad arguments return MHPPO_EINVAL and an empty request MHPPO_OK before any HIP call."""
    from mhppo import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    for fn in (L.mhppo_philox_uniform, L.mhppo_philox_normal):
        assert fn(7, 0, p, -1, None) == EINVAL
        assert b"bad argument" in L.mhppo_last_error()
        assert fn(7, 0, None, 4, None) == EINVAL
        assert fn(7, 0, None, 0, None) == EINVAL
        assert fn(7, 0, p, 0, None) == OK
    f2 = L.mhppo_philox_normal_2d
    assert f2(7, 0, 1 << 40, p, -1, 2, None) == EINVAL
    assert f2(7, 0, 1 << 40, p, 2, -1, None) == EINVAL
    assert f2(7, 0, 1 << 40, None, 2, 2, None) == EINVAL
    assert f2(7, 0, 1 << 40, p, 0, 2, None) == OK
    assert f2(7, 0, 1 << 40, p, 2, 0, None) == OK
    fe = L.mhppo_libm_eval
    for fn in (-1, 3):
        assert fe(fn, 0, 4, p, None) == EINVAL
        assert fe(fn, 0, 0, p, None) == EINVAL
    for fn in (0, 1, 2):
        assert fe(fn, 0, -1, p, None) == EINVAL
        assert fe(fn, 0, 4, None, None) == EINVAL
        assert fe(fn, 0, 0, p, None) == OK
    assert list(buf) == [0.0] * 4
