// block_prims.h — the block-level primitives of the small kernels (device): the one copy of the
// fixed-order float64 fold and of the ballot rank that the loss sums (ppo_loss.hip), the bucket
// plan and the scatter's reward sums (ppo_batch.hip), the diagnostics (mlp_infer.hip), the
// evaluation statistics (eval_stats.hip), the clip-and-Adam step's gradient norm (adam_clip.hip) and
// the head lists / record ranks (rollout_lists.h) use.
// Every sum these kernels make is "the same bits twice and on any stream"; the order that gives
// those bits is written down here and nowhere else (tests/fold_ref.py restates it in numpy,
// tests/test_fold_order_gpu.py pins it to the bit).
//
// The order of a fold over NT threads with CHAINS chains (k_fold, or strided_sum + block_sum):
//   1. thread b's chain u (u < CHAINS, CHAINS 1 or 4) starts at +0.0 and adds elements
//      b + u NT, b + u NT + CHAINS NT, b + u NT + 2 CHAINS NT, ... in ascending order;
//   2. four chains combine as (a0 + a1) + (a2 + a3);
//   3. the halving tree: sh[t] += sh[t + s] for every t < s, for s = NT/2, NT/4, ... 1; sh[0] is the sum.
// The order depends on n, NT and CHAINS alone, never on the grid or on scheduling.
//
// The order of a rank (block_rank): thread t's rank is the number of flagged threads before it in
// the block — the waves before its own in index order, then the lanes below its own (ballot,
// popcount) — so ranks ascend with the thread index and the placed lists are stable.
//
// The kernel here lives in an anonymous namespace (as mlp_grad_reduce.h's): every translation
// unit that includes this header instantiates its own.  All primitives are called by every thread
// of the block (they hold barriers) and use LDS of their own; two calls of the SAME instantiation
// in one kernel share that LDS, so they need a barrier between them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// v[k] <- the sum over the block's NT threads of their v[k], for NV values at once (one set of
// barriers), in the tree order above.  T: double or int.  Every thread gets the sums.
template <int NT, int NV, typename T>
__device__ __forceinline__ void block_sum(T (&v)[NV]) {
  static_assert(NT >= 64 && (NT & (NT - 1)) == 0, "block_sum: NT is a power of two");
  __shared__ T sh[NV][NT];
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NV; k++) sh[k][t] = v[k];
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s)
#pragma unroll
      for (int k = 0; k < NV; k++) sh[k][t] += sh[k][t + s];
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NV; k++) v[k] = sh[k][0];
}

// Thread b's part of the sum of p[0 .. n): steps 1 and 2 of the fold's order.
template <int NT, int CHAINS>
__device__ __forceinline__ double strided_sum(const double *__restrict__ p, int n) {
  static_assert(CHAINS == 1 || CHAINS == 4, "strided_sum: one chain or four");
  double a[CHAINS];
#pragma unroll
  for (int u = 0; u < CHAINS; u++) a[u] = 0.0;
  for (int b = threadIdx.x; b < n; b += CHAINS * NT)
#pragma unroll
    for (int u = 0; u < CHAINS; u++)
      if (b + u * NT < n) a[u] += p[b + u * NT];
  if constexpr (CHAINS == 4) return (a[0] + a[1]) + (a[2] + a[3]);
  else return a[0];
}

// The same part of the sum of f(0) .. f(n - 1): the mapped-element form (f: int -> double, called
// once per element, in the chain's order), for terms that are computed rather than stored.
template <int NT, int CHAINS, typename F>
__device__ __forceinline__ double strided_sum(F f, int n) {
  static_assert(CHAINS == 1 || CHAINS == 4, "strided_sum: one chain or four");
  double a[CHAINS];
#pragma unroll
  for (int u = 0; u < CHAINS; u++) a[u] = 0.0;
  for (int b = threadIdx.x; b < n; b += CHAINS * NT)
#pragma unroll
    for (int u = 0; u < CHAINS; u++)
      if (b + u * NT < n) a[u] += f(b + u * NT);
  if constexpr (CHAINS == 4) return (a[0] + a[1]) + (a[2] + a[3]);
  else return a[0];
}

// out[k] (+)= the fold of partials[k n .. (k + 1) n), k = blockIdx.x: one block of NT threads per
// array.  ADD: added to out[k], else written.  One chain serves a few hundred partials; four chains
// keep a thread's loads four deep for many (the bucket scatter's two per block, 20 480 blocks at
// 65 536 envs x 4 slots: one serial chain of n / 256 was 34 us there).
template <int NT, int CHAINS, bool ADD>
__global__ void __launch_bounds__(NT) k_fold(const double *__restrict__ partials, int n, double *out) {
  double v[1] = {strided_sum<NT, CHAINS>(partials + (size_t)blockIdx.x * n, n)};
  block_sum<NT>(v);
  if (threadIdx.x == 0) {
    if (ADD) out[blockIdx.x] += v[0];
    else out[blockIdx.x] = v[0];
  }
}

// For NF flags at once (one barrier): before[k] = the threads before this one in the block whose
// flag k is set, total[k] = all of the block's, in the rank order above.
template <int NT, int NF>
__device__ __forceinline__ void block_rank(const bool (&f)[NF], int (&before)[NF], int (&total)[NF]) {
  static_assert(NT % 64 == 0, "block_rank: whole waves");
  __shared__ int wsum[NF][NT / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint64_t m[NF];
#pragma unroll
  for (int k = 0; k < NF; k++) {
    m[k] = __ballot(f[k]);
    if (lane == 0) wsum[k][w] = __popcll(m[k]);
  }
  __syncthreads();
  const uint64_t below = lane ? ((1ull << lane) - 1) : 0ull;
#pragma unroll
  for (int k = 0; k < NF; k++) {
    int b = 0, a = 0;
#pragma unroll
    for (int q = 0; q < NT / 64; q++) {
      if (q < w) b += wsum[k][q];
      a += wsum[k][q];
    }
    before[k] = b + __popcll(m[k] & below);
    total[k] = a;
  }
}

}  // namespace
