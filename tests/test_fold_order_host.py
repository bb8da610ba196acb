"""The inputs of tests/test_fold_order_gpu.py have power: for every length the GPU tests fold
(the env counts of the evaluation statistics, the scatter's partial counts), over 33 arrays of
normal * exp(normal(0, 3)) at least one sum's BITS differ between the reference order
(fold_ref.fold at 1024 threads x 4 chains) and each wrong order.  Floors per wrong order: where a
CPU check with exactly such inputs showed differing sums (out of 33: sequential 29 at n = 255;
one chain of 256 16 at n = 1023; ((a0 + a1) + a2) + a3 16 at n = 4095).  Below 3 * 1024 + 2 elements a
fourth chain of zeros makes both combinations exact, so that variant (and one chain of 1024, the
same order up to n = 4096) is asserted from 4095 up."""
import numpy as np
import pytest

import fold_ref as F

LENGTHS = sorted(set(F.EVS_N) | {F.scatter_blocks(NS, T) for NS, T in F.SCATTER_NS_T})


def differ(a, b):
    return int((a.view(np.int64) != b.view(np.int64)).sum())


@pytest.mark.parametrize("n", LENGTHS)
def test_inputs_tell_the_orders_apart(n):
    x = F.heavy(np.random.default_rng(n), (33, n))
    ref = F.fold(x, 1024, 4)
    wrong = {}
    if n >= 255:
        wrong["sequential"] = F.sequential(x)
    if n >= 1023:
        wrong["one chain of 256"] = F.fold(x, 256, 1)
    if n >= 4095:
        wrong["one chain of 1024"] = F.fold(x, 1024, 1)
        wrong["((a0+a1)+a2)+a3"] = F.fold(x, 1024, 4, combine="left")
    for name, w in wrong.items():
        d = differ(ref, w)
        print(f"n {n}: {name}: {d} of 33 sums differ")
        assert d >= 1, name
        assert np.allclose(ref, w, rtol=1e-9, atol=1e-9 * np.abs(x).sum(-1).max()), name  # the same sum, another order


def test_reference_pieces():
    """The restatements agree with plainly written loops on small cases."""
    rng = np.random.default_rng(1)
    v = F.heavy(rng, 8)
    assert F.tree(v, 8) == ((v[0] + v[4]) + (v[2] + v[6])) + ((v[1] + v[5]) + (v[3] + v[7]))
    x = F.heavy(rng, 19)  # NT = 2, CHAINS = 4: thread b takes b, b + 2, b + 4, b + 6, then + 8
    a = [[0.0] * 4 for _ in range(2)]
    for b0 in range(0, 19, 8):
        for t in range(2):
            for u in range(4):
                if b0 + t + 2 * u < 19:
                    a[t][u] += x[b0 + t + 2 * u]
    th = [(a[t][0] + a[t][1]) + (a[t][2] + a[t][3]) for t in range(2)]
    assert F.fold(x, 2, 4) == th[0] + th[1]
    assert F.fold(x[:5], 256, 1) == F.tree(np.concatenate([x[:5], np.zeros(251)]), 256)
    w = F.heavy(rng, 64)
    s = w.copy()
    for m in (32, 16, 8, 4, 2, 1):
        s = np.array([s[l] + s[l ^ m] for l in range(64)])
    assert F.butterfly64(w) == s[0]
