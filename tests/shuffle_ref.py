"""An independent restatement of the minibatch shuffle (csrc/batch_shuffle.h), in plain numpy on
tests/philox_ref.py, written from the definition:

  h = max(1, ceil(bitlen(M - 1) / 2)), mask = 2^h - 1; the walk domain is 4^h
  round keys: the four Philox words of counter 0 under `key`, then those of counter 1
  one pass: (L, R) = (x >> h, x & mask); 8 rounds (L, R) <- (R, L ^ (fmix32(R ^ k_r) & mask)); x = L << h | R
  fmix32 (murmur3's finaliser): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
  perm(key, M, i): the pass applied to i, and again while the result is >= M
  slice bounds: b_j = 4 floor(j ceil(M / 4) / K) for j < K, b_K = M

`rounds` and `keys` exist for the wrong variants of the power test.  The module also holds the
statistics of the uniformity check and the shuffle key of Algo_PPO(minibatches=K)."""
import numpy as np

import philox_ref as pr

_U = np.uint64
MASK32 = (1 << 32) - 1


def half_bits(M):
    return max(1, (int(M - 1).bit_length() + 1) // 2)


def round_keys(key):
    return [int(w) for c in (0, 1) for w in pr.words(key, c)]


def fmix32(x):
    x = x ^ (x >> _U(16))
    x = (x * _U(0x85EBCA6B)) & _U(MASK32)  # < 2^64: no wrap before the mask
    x = x ^ (x >> _U(13))
    x = (x * _U(0xC2B2AE35)) & _U(MASK32)
    return x ^ (x >> _U(16))


def feistel(x, h, keys, rounds=8):
    """One pass of the network over the uint64 array x (values < 4^h)."""
    mask = _U((1 << h) - 1)
    L, R = x >> _U(h), x & mask
    for r in range(rounds):
        L, R = R, L ^ (fmix32(R ^ _U(keys[r])) & mask)
    return (L << _U(h)) | R


def perm(key, M, rounds=8, keys=None, passes=False):
    """int64 [M]: destination row i's source row (passes=True: also the walk passes each i took)."""
    M = int(M)
    h = half_bits(M) if M > 0 else 1
    keys = round_keys(key) if keys is None else keys
    x = np.arange(M, dtype=_U)
    n = np.zeros(M, np.int64)
    todo = np.arange(M)
    while todo.size:
        x[todo] = feistel(x[todo], h, keys, rounds)
        n[todo] += 1
        todo = todo[x[todo] >= _U(M)]
    out = x.astype(np.int64)
    return (out, n) if passes else out


def bounds(M, K):
    """[K + 1] ints: b_0 .. b_K."""
    c = (M + 3) // 4
    return [4 * ((j * c) // K) for j in range(K)] + [M]


# ---------------------------------------------------------------- the uniformity statistics
def chi2_slices(p, K=8):
    """chi^2 against independence of the K x K table (destination slice of K) x (source K-tile: the
    source row's floor(s K / M)), (K - 1)^2 degrees of freedom."""
    M = len(p)
    b = np.asarray(bounds(M, K))
    dst = np.searchsorted(b, np.arange(M), side="right") - 1
    src = (p * K) // M
    table = np.zeros((K, K))
    np.add.at(table, (dst, src), 1.0)
    exp = table.sum(1, keepdims=True) * table.sum(0, keepdims=True) / M
    return float(((table - exp) ** 2 / exp).sum())


def neighbour_fraction(p):
    """The fraction of neighbours i, i + 1 whose sources are neighbours too."""
    return float((np.abs(np.diff(p)) == 1).mean())


# ---------------------------------------------------------------- the product's shuffle key
SHUFFLE_TAG = 0x6D62736866666C65  # "mbshffle"
HEAD_INDEX = {"cross": 0, "wait": 1, "choice": 2}


def shuffle_key(seed, iteration, epoch, head, env0):
    """The key of one head's shuffle at one epoch (mhppo.shuffle.shuffle_key restated): the noise
    key seed * 1000003 + iteration of the iteration the batch was collected in, XOR a constant, plus
    (epoch, head index, the shard's first global env id) spread by odd multipliers, mod 2^64."""
    k = pr.noise_key(seed, iteration) ^ SHUFFLE_TAG
    k += (int(epoch) + 1) * 0x9E3779B97F4A7C15 + (int(head) + 1) * 0xC2B2AE3D27D4EB4F + int(env0) * 0x165667B19E3779F9
    return k & pr.MASK64
