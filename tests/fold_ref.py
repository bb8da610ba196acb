"""numpy restatements of the fixed summation orders of the small kernels (csrc/block_prims.h and
the kernels that feed it), for the tests that pin those orders to the bit.  Every function works
on float64 arrays with a leading batch of independent sums ([..., n]); numpy's elementwise float64
additions are the device's (IEEE, no contraction), so equal order means equal bits."""
import numpy as np


def heavy(rng, shape):
    """normal * exp(normal(0, 3)): magnitudes over many binades, so a sum's bits show its order."""
    return rng.standard_normal(shape) * np.exp(3.0 * rng.standard_normal(shape))


def tree(v, NT):
    """The LDS halving tree over NT threads: sh[t] += sh[t + s] for s = NT/2 .. 1."""
    v = np.array(v, dtype=np.float64)
    assert v.shape[-1] == NT and NT & (NT - 1) == 0
    s = NT // 2
    while s:
        v[..., :s] += v[..., s:2 * s]
        s //= 2
    return v[..., 0].copy()


def _chains(x, NT, CHAINS):
    """acc [..., CHAINS, NT]: element b + u NT (+ k CHAINS NT) of x goes to chain u of thread b."""
    x = np.asarray(x, dtype=np.float64)
    n, step = x.shape[-1], CHAINS * NT
    rounds = max(1, -(-n // step))
    # an absent element is skipped on the device; adding +0.0 to a chain that started at +0.0 is the same
    pad = np.zeros(x.shape[:-1] + (rounds * step,))
    pad[..., :n] = x
    pad = pad.reshape(x.shape[:-1] + (rounds, CHAINS, NT))
    acc = np.zeros(x.shape[:-1] + (CHAINS, NT))
    for r in range(rounds):
        acc = acc + pad[..., r, :, :]
    return acc


def strided(x, NT, CHAINS, combine="pairs"):
    """The per-thread value [..., NT] of the strided sum: CHAINS 1, or 4 combined as
    (a0 + a1) + (a2 + a3).  combine="left" is the WRONG order ((a0 + a1) + a2) + a3."""
    a = _chains(x, NT, CHAINS)
    if CHAINS == 1:
        return a[..., 0, :]
    assert CHAINS == 4
    if combine == "left":
        return ((a[..., 0, :] + a[..., 1, :]) + a[..., 2, :]) + a[..., 3, :]
    return (a[..., 0, :] + a[..., 1, :]) + (a[..., 2, :] + a[..., 3, :])


def fold(x, NT, CHAINS, combine="pairs"):
    """k_fold<NT, CHAINS, .>: the strided per-thread sums, then the tree.  [..., n] -> [...]"""
    return tree(strided(x, NT, CHAINS, combine), NT)


def sequential(x):
    """A WRONG order: plain left-to-right."""
    x = np.asarray(x, dtype=np.float64)
    acc = np.zeros(x.shape[:-1])
    for i in range(x.shape[-1]):
        acc = acc + x[..., i]
    return acc


def _blocks(v, NT):
    """[..., n] -> [..., ceil(n / NT), NT], the tail block padded with 0.0 (idle threads hold 0.0)."""
    n = v.shape[-1]
    nb = max(1, -(-n // NT))
    pad = np.zeros(v.shape[:-1] + (nb * NT,))
    pad[..., :n] = v
    return pad.reshape(v.shape[:-1] + (nb, NT))


def adv_stats(ret, val):
    """mhppo_adv_stats on float32 [M]: k_adv_stats' block partials (a = float32(ret - val); a and
    double(a)^2 through the 256-thread tree), folded by k_fold<256, 1, add> onto zeros.  -> float64 [2]"""
    a = (np.asarray(ret, np.float32) - np.asarray(val, np.float32)).astype(np.float32).astype(np.float64)
    part = tree(_blocks(np.stack([a, a * a]), 256), 256)  # [2, nblocks]
    return np.zeros(2) + fold(part, 256, 1)


def plan_ep_sum(ep_min, exist):
    """mhppo_bucket_plan's rew_sums[2]: k_plan_count's block partials of (double)(float)ep_min over
    the existing segments (256-thread tree), folded in k_plan_scan (256 threads, one chain)."""
    e = np.where(np.asarray(exist).reshape(-1) != 0, np.asarray(ep_min, np.float64).reshape(-1).astype(np.float32), 0)
    return fold(tree(_blocks(e.astype(np.float64), 256), 256), 256, 1)


def butterfly64(v):
    """A wave's 64-lane xor butterfly (a += shfl_xor(a, m) for m = 32 .. 1), lane 0's value.  [..., 64] -> [...]"""
    v = np.array(v, dtype=np.float64)
    lanes = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ m]
    return v[..., 0]


def scatter_partials(rew_tm, used, bucket):
    """k_bucket_scatter<true>'s partials at the default 1024-thread block.  rew_tm float64 [T, NS];
    used / bucket [NS]: the segment is bucketed (pos >= 0) / its bucket.  A block is 64 segments x
    16 steps, thread tid on segment tid % 64 of step tid / 64: each wave (one step) does the 64-lane
    butterfly, then the 16 waves are added in index order.  -> float64 [2, gridDim.y * gridDim.x],
    partial y * gridDim.x + x."""
    rew_tm = np.asarray(rew_tm, np.float64)
    T, NS = rew_tm.shape
    gx, gy = -(-NS // 64), -(-T // 16)
    r = np.zeros((gy * 16, gx * 64))
    r[:T, :NS] = rew_tm.astype(np.float32).astype(np.float64)
    out = np.zeros((2, gy, gx))
    for k in range(2):
        sel = np.zeros(gx * 64, bool)
        sel[:NS] = (np.asarray(used) != 0) & ((np.asarray(bucket) != 0) == bool(k))
        v = np.where(sel[None, :], r, 0.0).reshape(gy, 16, gx, 64)
        waves = butterfly64(v)  # [gy, 16, gx]
        a = np.zeros((gy, gx))
        for q in range(16):
            a = a + waves[:, q, :]
        out[k] = a
    return out.reshape(2, gy * gx)


def scatter_sums(rew_tm, used, bucket):
    """mhppo_bucket_scatter_sums' two sums: the partials folded by k_fold<1024, 4, add> onto the
    zeros k_plan_scan left.  -> float64 [2]"""
    return np.zeros(2) + fold(scatter_partials(rew_tm, used, bucket), 1024, 4)


# The shapes of tests/test_fold_order_gpu.py, shared with the CPU test of the inputs' power
# (tests/test_fold_order_host.py).
ADV_M = [1, 255, 256, 257, 256 * 255 + 1, 256 * 256, 256 * 256 + 1, 256 * 257 + 3]  # 256, 256, 257, 258 partials
EVS_N = [1, 1023, 1024, 1025, 4095, 4096, 4097, 8195]
SCATTER_NS_T = [(63, 2), (65, 2), (64 * 1024 + 1, 2), (64 * 4096 + 1, 2), (64 * 1025, 17)]


def scatter_blocks(NS, T):
    return -(-NS // 64) * -(-T // 16)
