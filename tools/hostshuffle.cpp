// hostshuffle.cpp — csrc/batch_shuffle.h compiled for the host: the minibatch shuffle's
// permutation, its round keys and the slice bounds, as the kernels compute them
// (tools/hostshuffle.py; tests/test_shuffle_host.py, tests/test_shuffle_gpu.py).
#include "../mh-ppo_amd/csrc/batch_shuffle.h"

using namespace mhppo;

extern "C" {

// out[i] = the source row of destination row i, i = 0 .. M - 1
void hs_perm(uint64_t key, int64_t M, uint32_t *out) {
  if (M < 1 || M > SHUFFLE_M_MAX) return;
  const ShuffleKeys s = shuffle_keys(key);
  const int h = shuffle_half_bits((uint32_t)M);
  for (int64_t i = 0; i < M; i++) out[i] = shuffle_perm(s, h, (uint32_t)M, (uint32_t)i);
}

void hs_keys(uint64_t key, uint32_t *out) {
  const ShuffleKeys s = shuffle_keys(key);
  for (int r = 0; r < SHUFFLE_ROUNDS; r++) out[r] = s.k[r];
}

int hs_half_bits(int64_t M) { return shuffle_half_bits((uint32_t)M); }

// out[j] = b_j, j = 0 .. K
void hs_bounds(int64_t M, int64_t K, int64_t *out) {
  for (int64_t j = 0; j <= K; j++) out[j] = shuffle_slice_bound(M, K, j);
}

}  // extern "C"
