// batch_shuffle.hip — the minibatch shuffle of one head's batch (+ C-ABI, mhppo_batch_shuffle; the
// contract is include/mhppo.h's): destination row i is source row shuffle_perm(key, M, i)
// (batch_shuffle.h), for X [M, n_in] and the three 4-byte columns act / logp / ret.
//
// k_batch_shuffle: a block of 256 threads owns a run of `rows` consecutive destination rows (256, or
// 128 for n_in > 32: at most 33 KB of LDS, eight blocks of 13-float rows per CU).
//   1. thread t computes the source row of destination row i0 + t (the cycle-walk: a wave waits for
//      its slowest lane, a few passes of 8 cheap rounds), keeps it in LDS and moves the row's three
//      column values itself (a 4-byte gather, a coalesced store);
//   2. the run's rows * n_in floats are read with adjacent lanes on adjacent floats of a source row
//      (13 of 16 lanes per row at n_in = 13: one contiguous 52-byte segment per row, five rows per
//      wave instruction; sources need only 4-byte alignment), four loads in flight per lane before
//      the first is used, into an LDS image of the destination run;
//   3. the image goes out as one contiguous span with 16-byte stores (i0 is a multiple of 4 rows, so
//      the span starts 16-byte aligned whatever n_in is), the last M n_in mod 4 floats one by one.
// Element e of the run is row e / n_in: a multiply-high with ceil(2^32 / n_in) (exact for
// e < 2^14), so n_in stays a run-time argument and there is one kernel.
//
// k_slice_counts: the choice head's per-slice action counts, one block per slice over the SHUFFLED
// act column, folded in block_prims.h's fixed order (no atomics; the terms are 0.0 / 1.0, so the
// sums are exact integers in any case).  A second small launch: the choice batch is at most N S rows.
#include <hip/hip_runtime.h>

#include "../../include/mhppo.h"
#include "batch_shuffle.h"
#include "block_prims.h"
#include "common.h"

using namespace mhppo;

namespace {

constexpr int NT = 256;
constexpr int DEPTH = 4;  // loads in flight per lane in step 2

__global__ void __launch_bounds__(NT)
    k_batch_shuffle(const ShuffleKeys keys, int h, uint32_t M, int n_in, uint32_t inv_n, int rows,
                    const float *__restrict__ X, const uint32_t *__restrict__ act, const uint32_t *__restrict__ logp,
                    const uint32_t *__restrict__ ret, float *__restrict__ dX, uint32_t *__restrict__ dact,
                    uint32_t *__restrict__ dlogp, uint32_t *__restrict__ dret) {
  extern __shared__ float4 lds4[];
  float *img = (float *)lds4;                         // [rows * n_in]
  uint32_t *src = (uint32_t *)(img + rows * n_in);    // [rows]
  const int t = threadIdx.x;
  const uint32_t i0 = blockIdx.x * (uint32_t)rows;
  const int nr = (int)(M - i0 < (uint32_t)rows ? M - i0 : (uint32_t)rows);
  if (t < nr) {
    const uint32_t s = shuffle_perm(keys, h, M, i0 + t);
    src[t] = s;
    const uint32_t a = act[s], l = logp[s], r = ret[s];
    dact[i0 + t] = a;
    dlogp[i0 + t] = l;
    dret[i0 + t] = r;
  }
  __syncthreads();
  const int ne = nr * n_in;
  for (int e0 = t; e0 < ne; e0 += DEPTH * NT) {
    float v[DEPTH];
#pragma unroll
    for (int u = 0; u < DEPTH; u++) {
      const int e = e0 + u * NT;
      if (e < ne) {
        const int r = n_in == 1 ? e : (int)__umulhi((uint32_t)e, inv_n);
        v[u] = X[(size_t)src[r] * n_in + (e - r * n_in)];
      }
    }
#pragma unroll
    for (int u = 0; u < DEPTH; u++)
      if (e0 + u * NT < ne) img[e0 + u * NT] = v[u];
  }
  __syncthreads();
  float *out = dX + (size_t)i0 * n_in;
  const int nv = ne >> 2;
  for (int q = t; q < nv; q += NT) ((float4 *)out)[q] = lds4[q];
  for (int e = 4 * nv + t; e < ne; e += NT) out[e] = img[e];
}

__global__ void __launch_bounds__(NT) k_slice_counts(const int32_t *__restrict__ act, int64_t M, int K, double *counts) {
  const int64_t b0 = shuffle_slice_bound(M, K, blockIdx.x), b1 = shuffle_slice_bound(M, K, blockIdx.x + 1);
  const int32_t *p = act + b0;
  const int n = (int)(b1 - b0);
  double v[2] = {strided_sum<NT, 4>([&](int i) { return p[i] == 0 ? 1.0 : 0.0; }, n),
                 strided_sum<NT, 4>([&](int i) { return p[i] == 1 ? 1.0 : 0.0; }, n)};
  block_sum<NT>(v);
  if (threadIdx.x == 0) {
    counts[2 * blockIdx.x] = v[0];
    counts[2 * blockIdx.x + 1] = v[1];
  }
}

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

}  // namespace

extern "C" int mhppo_batch_shuffle(int32_t n_in, int64_t M, const float *X, const void *act, const float *logp,
                                   const float *ret, uint64_t key, int32_t K, float *X_out, void *act_out,
                                   float *logp_out, float *ret_out, double *counts, void *stream) {
  if (n_in < 1 || n_in > 64) return set_error(MHPPO_EINVAL, "batch_shuffle: n_in %d outside 1 .. 64", n_in);
  if (K < 1) return set_error(MHPPO_EINVAL, "batch_shuffle: K %d < 1", K);
  if (M < 0 || M > SHUFFLE_M_MAX) return set_error(MHPPO_EINVAL, "batch_shuffle: M outside 0 .. 2^31 - 1");
  if (counts && M > ((int64_t)1 << 30))  // the fold's element index b + u NT stays in int
    return set_error(MHPPO_EINVAL, "batch_shuffle: counts need M <= 2^30");
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) {
    if (counts) CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)K * 2 * sizeof(double), st));
    return MHPPO_OK;
  }
  if (!X || !act || !logp || !ret || !X_out || !act_out || !logp_out || !ret_out)
    return set_error(MHPPO_EINVAL, "batch_shuffle: a NULL source or destination");
  const void *srcs[4] = {X, act, logp, ret};
  void *dsts[4] = {X_out, act_out, logp_out, ret_out};
  const size_t bytes[4] = {(size_t)M * n_in * 4, (size_t)M * 4, (size_t)M * 4, (size_t)M * 4};
  for (int a = 0; a < 4; a++) {
    if ((uintptr_t)srcs[a] % 4) return set_error(MHPPO_EINVAL, "batch_shuffle: a source is not 4-byte aligned");
    if ((uintptr_t)dsts[a] % 16) return set_error(MHPPO_EINVAL, "batch_shuffle: a destination is not 16-byte aligned");
  }
  for (int a = 0; a < 4; a++)
    for (int b = 0; b < 4; b++)
      if (overlap(srcs[a], bytes[a], dsts[b], bytes[b]))
        return set_error(MHPPO_EINVAL, "batch_shuffle: a source overlaps a destination");
  const int rows = n_in > 32 ? 128 : 256;
  const uint32_t inv_n = n_in == 1 ? 0u : (uint32_t)((((uint64_t)1 << 32) + n_in - 1) / n_in);
  const size_t lds = (size_t)rows * n_in * 4 + (size_t)rows * 4;
  const unsigned blocks = (unsigned)((M + rows - 1) / rows);
  hipLaunchKernelGGL(k_batch_shuffle, dim3(blocks), dim3(NT), lds, st, shuffle_keys(key),
                     shuffle_half_bits((uint32_t)M), (uint32_t)M, (int)n_in, inv_n, rows, X, (const uint32_t *)act,
                     (const uint32_t *)logp, (const uint32_t *)ret, X_out, (uint32_t *)act_out, (uint32_t *)logp_out,
                     (uint32_t *)ret_out);
  CHECK_HIP(hipGetLastError());
  if (counts) {
    hipLaunchKernelGGL(k_slice_counts, dim3(K), dim3(NT), 0, st, (const int32_t *)act_out, M, (int)K, counts);
    CHECK_HIP(hipGetLastError());
  }
  return MHPPO_OK;
}
