"""The minibatch shuffle (opt-in, Algo_PPO(minibatches=K); beyond the reference, whose epochs are
full-batch): a stateless keyed bijection of [0, M), the slice bounds of a shuffled batch, the key
of a head's shuffle, and shuffle_batch, the one caller of mhppo_batch_shuffle.

perm_torch restates the bijection of csrc/batch_shuffle.h (include/mhppo.h has the definition) in
int64 torch ops; plain indexing with it is the shuffle's specification and its CPU path (the gloo
test doubles), the role adam_clip_torch plays for the clip.  Nothing is drawn or sorted, and no
generator state exists: a shuffle is a pure function of (key, M), so a resumed run repeats it."""
import torch

from . import _lib

M_MAX = (1 << 31) - 1
_M32, _M64 = (1 << 32) - 1, (1 << 64) - 1


def _philox_words(seed, ctr):
    """The four Philox-4x32-10 words of counter `ctr` under `seed` (csrc/ppo_math.h philox_words),
    in Python integers: the shuffle needs eight words per call."""
    c = [ctr & _M32, (ctr >> 32) & _M32, 0x6D687070, 0]
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & _M32, (p0 >> 32) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c


def round_keys(key):
    key = int(key) & _M64
    return _philox_words(key, 0) + _philox_words(key, 1)


def half_bits(M):
    return max(1, (int(M - 1).bit_length() + 1) // 2)


def _fmix32(x):
    # int64 holding 32-bit values: a product wraps mod 2^64, which keeps its low 32 bits
    x = x ^ (x >> 16)
    x = (x * 0x85EBCA6B) & _M32
    x = x ^ (x >> 13)
    x = (x * 0xC2B2AE35) & _M32
    return x ^ (x >> 16)


def perm_torch(key, M, device="cpu"):
    """int64 [M]: destination row i's source row under `key`."""
    M = int(M)
    if not 0 <= M <= M_MAX:
        raise ValueError(f"M must lie in 0 .. 2^31 - 1, not {M}")
    x = torch.arange(M, dtype=torch.int64, device=device)
    if M == 0:
        return x
    h, keys = half_bits(M), round_keys(key)
    mask = (1 << h) - 1
    todo = torch.arange(M, dtype=torch.int64, device=device)
    while todo.numel():
        v = x[todo]
        L, R = v >> h, v & mask
        for k in keys:
            L, R = R, L ^ (_fmix32(R ^ k) & mask)
        v = (L << h) | R
        x[todo] = v
        todo = todo[v >= M]  # cycle-walk: the rows still outside [0, M) take another pass
    return x


def slice_bounds(M, K):
    """[b_0 .. b_K]: slice j of K holds the shuffled rows [b_j, b_{j+1}); b_j = 4 floor(j ceil(M / 4) / K),
    b_K = M.  Every slice starts at a multiple of 4 rows; slices are empty when M < 4 K."""
    c = (int(M) + 3) // 4
    return [4 * ((j * c) // K) for j in range(K)] + [int(M)]


SHUFFLE_TAG = 0x6D62736866666C65  # "mbshffle": no shuffle key is a noise key (seed * 1000003 + iteration)
HEAD_INDEX = {"cross": 0, "wait": 1, "choice": 2}


def shuffle_key(seed, iteration, epoch, head, env0):
    """The key of one head's shuffle at one epoch, a pure function of its arguments:
    ((seed * 1000003 + iteration) mod 2^64 ^ SHUFFLE_TAG) + (epoch + 1) * 0x9E3779B97F4A7C15
    + (head + 1) * 0xC2B2AE3D27D4EB4F + env0 * 0x165667B19E3779F9, mod 2^64.
    seed, iteration: RolloutGPU.draw_noise's key scheme, for the iteration the batch was collected in;
    head: HEAD_INDEX (0 cross, 1 wait, 2 choice, fixed by name whichever heads an iteration trains);
    env0: the first global env id of this rank's shard (ranks draw different permutations)."""
    k = ((int(seed) * 1000003 + int(iteration)) & _M64) ^ SHUFFLE_TAG
    k += (int(epoch) + 1) * 0x9E3779B97F4A7C15 + (int(head) + 1) * 0xC2B2AE3D27D4EB4F + int(env0) * 0x165667B19E3779F9
    return k & _M64


def shuffle_batch(src, dst, key, K, counts=None):
    """dst <- src shuffled under `key`: src / dst = (obs [M, n_in] float32, act [M] float32 or
    int32, logp [M], ret [M] float32), contiguous; dst row i is src row perm(key, M, i).
    counts: None, or float64 [K, 2], written with each slice's rows with act == 0 / == 1 (act int32).
    GPU: one mhppo_batch_shuffle call on the current stream (plus the small counts launch); CPU
    tensors: indexing with perm_torch, the specification."""
    obs, act, logp, ret = src
    M, n_in = obs.shape
    K = int(K)
    if obs.device.type == "cuda":
        a = [t.data_ptr() if M else None for t in (*src, *dst)]
        with torch.cuda.device(obs.device):
            _lib.batch_shuffle(n_in, M, a[0], a[1], a[2], a[3], key, K, a[4], a[5], a[6], a[7],
                               None if counts is None else counts.data_ptr(),
                               torch.cuda.current_stream(obs.device).cuda_stream)
        return
    p = perm_torch(key, M)
    for s, d in zip(src, dst):
        d.copy_(s[p])
    if counts is not None:
        b = slice_bounds(M, K)
        for j in range(K):
            a = dst[1][b[j]:b[j + 1]]
            counts[j, 0], counts[j, 1] = float((a == 0).sum()), float((a == 1).sum())
