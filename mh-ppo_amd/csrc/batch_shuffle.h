// batch_shuffle.h — the minibatch shuffle's definitions (host+device): a stateless keyed bijection
// of [0, M) and the slice bounds of a shuffled batch.  No index array is built or sorted:
// shuffle_perm(keys, h, M, i) is computed where it is needed (csrc/batch_shuffle.hip per destination
// row, tools/hostshuffle.cpp on the host; tests/shuffle_ref.py restates it in numpy and
// mhppo/shuffle.py in torch).
//
//   h = max(1, ceil(bitlen(M - 1) / 2)), mask = 2^h - 1: the walk domain is 4^h >= M (< 4 M for M >= 2)
//   round keys k_0 .. k_7: the four words of philox_words(key, 0), then those of philox_words(key, 1)
//   one pass: (L, R) = (x >> h, x & mask); 8 times (L, R) <- (R, L ^ (fmix32(R ^ k_r) & mask));
//             x = L << h | R        (a balanced Feistel network: a bijection of [0, 4^h))
//   cycle-walk: the pass is applied again while its result is >= M (a bijection of [0, M): the walk
//             follows the network's cycle through i until it re-enters [0, M))
#pragma once
#include "ppo_math.h"

namespace mhppo {

constexpr int SHUFFLE_ROUNDS = 8;
constexpr int64_t SHUFFLE_M_MAX = ((int64_t)1 << 31) - 1;  // x stays in 32 bits (h <= 16)

struct ShuffleKeys {
  uint32_t k[SHUFFLE_ROUNDS];
};

MHPPO_HD inline ShuffleKeys shuffle_keys(uint64_t key) {
  ShuffleKeys s;
  philox_words(key, 0, s.k);
  philox_words(key, 1, s.k + 4);
  return s;
}

// half the walk domain's bits, for 1 <= M <= SHUFFLE_M_MAX
MHPPO_HD inline int shuffle_half_bits(uint32_t M) {
  int bits = 0;
  for (uint32_t v = M - 1; v; v >>= 1) bits++;
  const int h = (bits + 1) / 2;
  return h < 1 ? 1 : h;
}

// the murmur3 finaliser
MHPPO_HD inline uint32_t fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// destination row i's source row, i < M; h = shuffle_half_bits(M)
MHPPO_HD inline uint32_t shuffle_perm(const ShuffleKeys &s, int h, uint32_t M, uint32_t i) {
  const uint32_t mask = (1u << h) - 1u;
  uint32_t x = i;
  do {
    uint32_t L = x >> h, R = x & mask;
#pragma unroll
    for (int r = 0; r < SHUFFLE_ROUNDS; r++) {
      const uint32_t t = L ^ (fmix32(R ^ s.k[r]) & mask);
      L = R;
      R = t;
    }
    x = (L << h) | R;
  } while (x >= M);
  return x;
}

// Slice j of K covers the shuffled rows [b_j, b_{j+1}): b_j = 4 floor(j ceil(M / 4) / K) for j < K,
// b_K = M.  Every slice starts at a multiple of 4 rows (16-byte aligned rows of 13 floats, as the
// wait bucket's first row is); slices are empty when M < 4 K.
MHPPO_HD inline int64_t shuffle_slice_bound(int64_t M, int64_t K, int64_t j) {
  if (j >= K) return M;
  return 4 * ((j * ((M + 3) / 4)) / K);
}

}  // namespace mhppo
