"""ctypes wrapper of tools/libhostshuffle.so: csrc/batch_shuffle.h compiled for the CPU (the
minibatch shuffle's permutation, round keys and slice bounds).  numpy out."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
L = ctypes.CDLL(os.path.join(HERE, "libhostshuffle.so"))
P, I64, U64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64
for _name, _res, _args in (("hs_perm", None, [U64, I64, P]), ("hs_keys", None, [U64, P]),
                           ("hs_half_bits", ctypes.c_int, [I64]), ("hs_bounds", None, [I64, I64, P])):
    getattr(L, _name).restype = _res
    getattr(L, _name).argtypes = _args
_M64 = (1 << 64) - 1


def perm(key, M):
    """uint32 [M]: destination row i's source row."""
    out = np.zeros(M, np.uint32)
    L.hs_perm(int(key) & _M64, M, out.ctypes.data_as(P))
    return out


def keys(key):
    out = np.zeros(8, np.uint32)
    L.hs_keys(int(key) & _M64, out.ctypes.data_as(P))
    return out


def half_bits(M):
    return int(L.hs_half_bits(M))


def bounds(M, K):
    """int64 [K + 1]: b_0 .. b_K."""
    out = np.zeros(K + 1, np.int64)
    L.hs_bounds(M, K, out.ctypes.data_as(P))
    return out
