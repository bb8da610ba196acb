"""mhppo_batch_shuffle on the GPU (csrc/batch_shuffle.hip) against indexing with the numpy
restatement of the permutation (tests/shuffle_ref.py), bit for bit: every row-count / width path of
the kernel, the bitwise copy of the act column, the per-slice counts, a source that is only 4-byte
aligned, determinism across calls and streams, and the ABI's error cases (which write nothing).
All comparisons are of the 32-bit patterns; every destination sits between sentinel words that
must survive."""
import numpy as np
import pytest
import torch

import shuffle_ref as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MS = (0, 1, 3, 4, 5, 63, 64, 65, 257, 4099)
N_INS = (13, 27, 54, 64)
KS = (1, 3, 7)
KEY = (0xC0FFEE << 32) | 12345
PAD = 64          # sentinel words on either side of a destination (256 bytes: 16-byte alignment kept)
SENT = 0x5A5A5A5A
EINVAL = -1


def _lib():
    from mhppo import _lib
    return _lib


def _bits(M, n_in, seed, choice=False):
    """Source arrays as int32 bit patterns: X [M, n_in], act, logp, ret [M].  A float act carries
    NaN payloads, -0.0 and infinities; a choice act is 0 / 1 (and a few other values, counted by
    neither column)."""
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 3, (M, n_in)).astype(np.float32).view(np.int32)
    if choice:
        act = rng.integers(0, 2, M).astype(np.int32)
        act[rng.uniform(size=M) < 0.05] = 2
    else:
        act = rng.normal(-1, 1, M).astype(np.float32).view(np.int32)
        special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x7F800000, 0x00000001], np.uint32)
        idx = rng.uniform(size=M) < 0.3
        act[idx] = rng.choice(special, int(idx.sum())).view(np.int32)
    logp = rng.normal(-0.6, 0.3, M).astype(np.float32).view(np.int32)
    ret = rng.normal(-20, 8, M).astype(np.float32).view(np.int32)
    return X, act, logp, ret


class Dst:
    """A destination of n words between two PAD-word sentinels, 16-byte aligned."""

    def __init__(self, n, stream_dev=DEV):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), SENT, dtype=torch.int32, device=stream_dev)
        assert (self.buf.data_ptr() + 4 * PAD) % 16 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD

    def body(self):
        return self.buf[PAD:PAD + self.n].cpu().numpy()

    def intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:PAD] == SENT).all() and (b[PAD + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.buf.cpu().numpy() == SENT).all())


def _call(n_in, M, src, key, K, dst, counts=None, stream=None):
    L = _lib()
    st = torch.cuda.current_stream(DEV) if stream is None else stream
    return L.lib().mhppo_batch_shuffle(n_in, M, *[s if isinstance(s, int) else s.data_ptr() for s in src], key, K,
                                       *[d if isinstance(d, int) else d.ptr for d in dst],
                                       None if counts is None else counts.data_ptr(), st.cuda_stream)


def _run(n_in, M, bits, key, K, counts=None, stream=None, offset_rows=0):
    """The shuffle of `bits` (host arrays) on the GPU: (the four destination bodies, the Dst objects).
    offset_rows: the sources start that many 13-float rows into a larger allocation (4-byte aligned
    only)."""
    src = []
    for a in bits:
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        if offset_rows:
            big = torch.full((t.numel() + 13 * offset_rows + 3,), SENT, dtype=torch.int32, device=DEV)
            big[13 * offset_rows:13 * offset_rows + t.numel()] = t.reshape(-1)
            t = big[13 * offset_rows:13 * offset_rows + t.numel()]
            assert t.data_ptr() % 16 != 0 and t.data_ptr() % 4 == 0
        src.append(t)
    dst = [Dst(M * n_in), Dst(M), Dst(M), Dst(M)]
    assert _call(n_in, M, src, key, K, dst, counts, stream) == 0, _lib().lib().mhppo_last_error()
    (stream or torch.cuda.current_stream(DEV)).synchronize()
    return [d.body() for d in dst], dst


def _want(bits, key, M):
    p = sr.perm(key, M)
    return [a[p] for a in bits]


@pytest.mark.parametrize("n_in", N_INS)
def test_shuffle_equals_indexing(n_in):
    for M in MS:
        bits = _bits(M, n_in, seed=M + n_in)
        want = _want(bits, KEY, M)
        for K in KS:
            got, dst = _run(n_in, M, bits, KEY, K)
            for g, w, d in zip(got, want, dst):
                assert np.array_equal(g, w.reshape(-1)), (n_in, M, K)
                assert d.intact(), (n_in, M, K)


def test_act_copy_is_bitwise():
    M = 4099
    bits = _bits(M, 13, seed=1)
    act = bits[1].view(np.uint32)
    assert (act == 0x80000000).any() and (act == 0xFFC12345).any() and (act == 0x7FC00001).any()
    got, _ = _run(13, M, bits, 77, 3)
    assert np.array_equal(got[1], bits[1][sr.perm(77, M)])


@pytest.mark.parametrize("n_in", (27, 64))
def test_counts_per_slice(n_in):
    for M in MS:
        bits = _bits(M, n_in, seed=3 * M + 1, choice=True)
        want = _want(bits, KEY + M, M)
        for K in KS:
            counts = torch.full((K + 1, 2), -7.0, dtype=torch.float64, device=DEV)
            got, dst = _run(n_in, M, bits, KEY + M, K, counts=counts)
            assert all(np.array_equal(g, w.reshape(-1)) for g, w in zip(got, want))
            b = sr.bounds(M, K)
            c = counts.cpu().numpy()
            for j in range(K):
                a = want[1][b[j]:b[j + 1]]
                assert c[j].tolist() == [float((a == 0).sum()), float((a == 1).sum())], (n_in, M, K, j)
            assert c[K].tolist() == [-7.0, -7.0]  # nothing past counts[K][2]


def test_source_only_4_byte_aligned():
    for M in (5, 257, 4099):
        bits = _bits(M, 13, seed=M)
        got, dst = _run(13, M, bits, KEY, 3, offset_rows=1)
        for g, w, d in zip(got, _want(bits, KEY, M), dst):
            assert np.array_equal(g, w.reshape(-1)) and d.intact()


def test_same_bytes_twice_and_on_a_side_stream():
    M, n_in, K = 4099, 27, 7
    bits = _bits(M, n_in, seed=5, choice=True)
    outs = []
    side = torch.cuda.Stream(device=DEV)
    for stream in (None, None, side):
        counts = torch.zeros(K, 2, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        got, _ = _run(n_in, M, bits, KEY, K, counts=counts, stream=stream)
        outs.append([g.tobytes() for g in got] + [counts.cpu().numpy().tobytes()])
    assert outs[0] == outs[1] == outs[2]


def test_keys_give_different_outputs():
    M = 257
    bits = _bits(M, 13, seed=9)
    a, _ = _run(13, M, bits, 1, 1)
    b, _ = _run(13, M, bits, 2, 1)
    c, _ = _run(13, M, bits, 1 + (1 << 32), 1)  # the key's high word counts
    assert not np.array_equal(a[0], b[0]) and not np.array_equal(a[0], c[0]) and not np.array_equal(b[3], c[3])


def test_einval_cases_write_nothing():
    M, n_in, K = 65, 13, 3
    bits = _bits(M, n_in, seed=2, choice=True)
    src = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in bits]

    def fresh():
        return [Dst(M * n_in), Dst(M), Dst(M), Dst(M)]

    def refused(rc, dst, counts=None):
        torch.cuda.synchronize()
        assert rc == EINVAL, rc
        assert all(d.untouched() for d in dst if isinstance(d, Dst))
        if counts is not None:
            assert (counts.cpu().numpy() == -7.0).all()

    counts = torch.full((K, 2), -7.0, dtype=torch.float64, device=DEV)
    for bad_n in (0, 65, -1):
        d = fresh()
        refused(_call(bad_n, M, src, KEY, K, d, counts), d, counts)
    for bad_k in (0, -2):
        d = fresh()
        refused(_call(n_in, M, src, KEY, bad_k, d, counts), d, counts)
    d = fresh()
    refused(_call(n_in, -1, src, KEY, K, d, counts), d, counts)
    d = fresh()
    refused(_call(n_in, 1 << 31, src, KEY, K, d, counts), d, counts)
    for k in range(4):  # a NULL source, a NULL destination
        d = fresh()
        refused(_call(n_in, M, [0 if i == k else s for i, s in enumerate(src)], KEY, K, d, counts), d, counts)
        d = fresh()
        refused(_call(n_in, M, src, KEY, K, [0 if i == k else x for i, x in enumerate(d)], counts), d, counts)
    for k in range(4):  # a destination off 16 bytes, a source off 4 bytes
        d = fresh()
        refused(_call(n_in, M, src, KEY, K, [x.ptr + 4 if i == k else x for i, x in enumerate(d)], counts), d, counts)
        d = fresh()
        refused(_call(n_in, M, [s.data_ptr() + 2 if i == k else s for i, s in enumerate(src)], KEY, K, d, counts), d,
                counts)
    # a source aliasing a destination: in place, and overlapping by one 16-byte step
    before = [s.clone() for s in src]
    for k in range(4):
        d = fresh()
        refused(_call(n_in, M, src, KEY, K, [src[k].data_ptr() if i == k else x for i, x in enumerate(d)], counts), d,
                counts)
    big = torch.full((2 * M * n_in + 8,), SENT, dtype=torch.int32, device=DEV)
    big[:M * n_in] = src[0].reshape(-1)
    d = fresh()
    rc = _call(n_in, M, [big.data_ptr()] + src[1:], KEY, K, [big.data_ptr() + 4 * (M * n_in - 4)] + d[1:], counts)
    refused(rc, d[1:], counts)
    assert (big[M * n_in:].cpu().numpy() == SENT).all()
    assert all(torch.equal(a, b) for a, b in zip(before, src))
    # the same call, valid, goes through (the refusals above were about their arguments)
    d = fresh()
    assert _call(n_in, M, src, KEY, K, d, counts) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d[0].body(), bits[0][sr.perm(KEY, M)].reshape(-1))


def test_m0_zeroes_counts_and_launches_nothing():
    counts = torch.full((3, 2), -7.0, dtype=torch.float64, device=DEV)
    assert _call(13, 0, [0, 0, 0, 0], KEY, 3, [0, 0, 0, 0], counts) == 0
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == 0.0).all()


def test_shuffle_batch_wrapper():
    """mhppo.shuffle.shuffle_batch on GPU tensors: the same rows as its CPU path (the specification)."""
    from mhppo import shuffle
    M, n_in, K = 257, 27, 3
    bits = _bits(M, n_in, seed=4, choice=True)
    src = (torch.from_numpy(bits[0].view(np.float32)), torch.from_numpy(bits[1]),
           torch.from_numpy(bits[2].view(np.float32)), torch.from_numpy(bits[3].view(np.float32)))
    out = []
    for dev in ("cpu", DEV):
        s = tuple(t.to(dev) for t in src)
        d = tuple(torch.empty_like(t) for t in s)
        counts = torch.zeros(K, 2, dtype=torch.float64, device=dev)
        shuffle.shuffle_batch(s, d, KEY, K, counts)
        out.append([t.cpu().numpy().tobytes() for t in d] + [counts.cpu().numpy().tobytes()])
    assert out[0] == out[1]
