"""The minibatch shuffle's definitions on the CPU (no GPU): csrc/batch_shuffle.h compiled for the
host (tools/hostshuffle.cpp) and mhppo.shuffle.perm_torch against tests/shuffle_ref.py, a numpy
restatement written from the definition; the bijection; the slice bounds; the uniformity of the
minibatches the permutation cuts; and the power of those checks against wrong variants."""
import os
import sys

import numpy as np
import pytest
import torch

import philox_ref as pr
import shuffle_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS = (1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 4099, 65537)
KEYS = (0, 7, 12345, (1 << 63) + 5, (0xDEADBEEF << 32) | 17)  # with and without a high word
KEYS3 = (3, (1 << 40) + 1, (1 << 64) - 1)
UNIFORM_MS = (65536, 65537, 100000, 65584)
CHI2_MAX = 120.0        # the 49-degrees-of-freedom quantile near 1e-6
NEIGHBOUR_MAX = 2e-4


def hostshuffle():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import hostshuffle as hs
    return hs


def test_round_keys_and_half_bits():
    hs = hostshuffle()
    from mhppo import shuffle
    for key in KEYS:
        want = [int(w) for c in (0, 1) for w in pr.words(key, c)]
        assert sr.round_keys(key) == want
        assert [int(x) for x in hs.keys(key)] == want
        assert shuffle.round_keys(key) == want
    for M, h in ((1, 1), (2, 1), (4, 1), (5, 2), (16, 2), (17, 3), (256, 4), (257, 5), (65536, 8), (65537, 9),
                 (10485760, 12), (2**31 - 1, 16)):
        assert sr.half_bits(M) == h and hs.half_bits(M) == h and shuffle.half_bits(M) == h
        assert 4 ** h >= M and (M < 2 or 4 ** h < 4 * M)


def test_fmix32_is_murmur3_finaliser():
    # murmur3's fmix32 fixes 0 and is a bijection of the 32-bit words; two published values
    x = np.array([0, 1, 0xFFFFFFFF], np.uint64)
    assert [int(v) for v in sr.fmix32(x)] == [0, 0x514E28B7, 0x81F16F39]


@pytest.mark.parametrize("key", KEYS)
def test_host_header_equals_restatement(key):
    hs = hostshuffle()
    for M in MS:
        want = sr.perm(key, M)
        got = hs.perm(key, M)
        assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), want), (key, M)


@pytest.mark.parametrize("key", KEYS)
def test_perm_torch_equals_restatement(key):
    from mhppo import shuffle
    for M in (0,) + MS:
        got = shuffle.perm_torch(key, M)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), sr.perm(key, M)), (key, M)


@pytest.mark.parametrize("key", KEYS3)
def test_bijection_up_to_700(key):
    hs = hostshuffle()
    for M in range(1, 701):
        p = hs.perm(key, M)
        assert np.array_equal(np.sort(p), np.arange(M)), (key, M)
        if M in (1, 2, 3, 7, 64, 65, 699, 700):
            assert np.array_equal(np.sort(sr.perm(key, M)), np.arange(M)), (key, M)


def test_keys_give_different_permutations():
    ps = [tuple(sr.perm(k, 257)) for k in KEYS]
    assert len(set(ps)) == len(KEYS)


def test_slice_bounds():
    hs = hostshuffle()
    from mhppo import shuffle
    for M in range(0, 71):
        for K in range(1, 10):
            b = sr.bounds(M, K)
            assert list(hs.bounds(M, K)) == b and shuffle.slice_bounds(M, K) == b
            assert len(b) == K + 1 and b[0] == 0 and b[K] == M
            assert all(b[j] <= b[j + 1] for j in range(K))
            assert all(b[j] % 4 == 0 for j in range(K))
            sizes = [b[j + 1] - b[j] for j in range(K)]
            assert max(sizes) - min(sizes) <= 4, (M, K, sizes)
    # the definition, at a size where j ceil(M / 4) passes 2^31
    M, K = 2**31 - 1, 7
    assert list(hs.bounds(M, K)) == [4 * ((j * ((M + 3) // 4)) // K) for j in range(K)] + [M]


def _uniformity(perm_of):
    """(max chi^2, max neighbour fraction) over 20 keys and UNIFORM_MS."""
    chi, nb = 0.0, 0.0
    for k in range(20):
        key = pr.noise_key(k, 3 * k) ^ sr.SHUFFLE_TAG
        for M in UNIFORM_MS:
            p = perm_of(key, M)
            chi, nb = max(chi, sr.chi2_slices(p, 8)), max(nb, sr.neighbour_fraction(p))
    return chi, nb


def test_uniformity():
    """Destination slice (K = 8) against source octile: chi^2 against independence at most 120 (49
    degrees of freedom, the quantile near 1e-6) in each of the 80 cases; at most 2e-4 of the
    neighbours i, i + 1 keep neighbouring sources.  The host-compiled header is what is measured."""
    hs = hostshuffle()
    chi, nb = _uniformity(lambda key, M: hs.perm(key, M).astype(np.int64))
    print(f"max chi^2 {chi:.1f}, max neighbour fraction {nb:.2e}")
    assert chi <= CHI2_MAX and nb <= NEIGHBOUR_MAX, (chi, nb)


def test_uniformity_checks_have_power():
    """One round, or all-zero round keys, fail the same checks."""
    chi, nb = _uniformity(lambda key, M: sr.perm(key, M, rounds=1))
    assert chi > CHI2_MAX or nb > NEIGHBOUR_MAX, (chi, nb)
    # all-zero keys at the full eight rounds (the network then fixes 0 and walks badly off 4^h)
    zero = [sr.perm(0, M, keys=[0] * 8) for M in UNIFORM_MS]
    chi0, nb0 = max(sr.chi2_slices(p, 8) for p in zero), max(sr.neighbour_fraction(p) for p in zero)
    assert chi0 > CHI2_MAX and nb0 > NEIGHBOUR_MAX, (chi0, nb0)
    # ... every key gives ONE permutation, and it differs from the header's index for index
    hs = hostshuffle()
    z = sr.perm(5, 4099, keys=[0] * 8)
    assert np.array_equal(z, sr.perm(6, 4099, keys=[0] * 8))
    assert not np.array_equal(z, hs.perm(5, 4099).astype(np.int64))


def test_shuffle_key():
    from mhppo import shuffle
    seen = set()
    for seed in (0, 1, 2**40):
        for it in (0, 1, 999):
            for e in range(10):
                for head in range(3):
                    for env0 in (0, 64, 65536):
                        k = shuffle.shuffle_key(seed, it, e, head, env0)
                        assert k == sr.shuffle_key(seed, it, e, head, env0) and 0 <= k < 2**64
                        seen.add(k)
    assert len(seen) == 3 * 3 * 10 * 3 * 3
    noise = {pr.noise_key(s, i) for s in (0, 1, 2**40) for i in range(2000)}
    assert not (seen & noise)
    assert shuffle.HEAD_INDEX == {"cross": 0, "wait": 1, "choice": 2}


def test_shuffle_batch_cpu_is_indexing():
    """The CPU path (the specification): plain indexing with perm_torch, and the per-slice counts."""
    from mhppo import shuffle
    rng = np.random.default_rng(0)
    M, K, key = 37, 3, 99
    src = (torch.from_numpy(rng.normal(size=(M, 5)).astype(np.float32)),
           torch.from_numpy(rng.integers(0, 2, M).astype(np.int32)),
           torch.from_numpy(rng.normal(size=M).astype(np.float32)), torch.from_numpy(rng.normal(size=M).astype(np.float32)))
    dst = tuple(torch.empty_like(t) for t in src)
    counts = torch.full((K, 2), -1.0, dtype=torch.float64)
    shuffle.shuffle_batch(src, dst, key, K, counts)
    p = sr.perm(key, M)
    b = sr.bounds(M, K)
    for s, d in zip(src, dst):
        assert np.array_equal(d.numpy(), s.numpy()[p])
    for j in range(K):
        a = src[1].numpy()[p][b[j]:b[j + 1]]
        assert counts[j].tolist() == [float((a == 0).sum()), float((a == 1).sum())]
