// rollout_lists.h — the index lists mhppo_rollout_begin builds once per episode, each by the same
// two passes (per-block counts, then every block sums the counts before it and places its rows by
// wave prefix; no block waits on another):
//   k_head_count / k_head_place   the head lists of k_policy_mfma: the cross rows, then the wait rows
//   k_flag_count / k_flag_rank    the compact record layout's ranks (mhppo_rollout_bufs.rec_of)
//   part_env / k_part_bounds      the env range of a rollout part and where its rows start in the lists
// Part of the rollout.hip translation unit (one anonymous namespace); not for inclusion elsewhere.
#pragma once
#include <algorithm>

#include "launch1d.h"
#include "rollout_dev.h"

namespace {
using namespace mhppo;

// Head lists for k_policy_sorted / k_policy_mfma (stable: each list in row order).  Pass 1 counts the
// cross rows of each 256-row block; pass 2 has every block sum the counts before it
// (and all of them, for the wait list's base), then place its rows by wave prefix.
// cnt[2 b] / cnt[2 b + 1]: block b's cross / wait rows.
__global__ void __launch_bounds__(TPB) k_head_count(const int32_t *a_d, int R, int32_t *cnt) {
  __shared__ int wsum[2][TPB / 64];
  const int r = blockIdx.x * TPB + threadIdx.x;
  const bool valid = r < R;
  const bool cross = valid && a_d[r] == 0;  // action_d = 2a - 1 <= 0 (:440-445)
  const uint64_t mc = __ballot(cross), mw = __ballot(valid && !cross);
  if ((threadIdx.x & 63) == 0) {
    wsum[0][threadIdx.x >> 6] = __popcll(mc);
    wsum[1][threadIdx.x >> 6] = __popcll(mw);
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    int s = 0;
    for (int w = 0; w < TPB / 64; w++) s += wsum[threadIdx.x][w];
    cnt[2 * blockIdx.x + threadIdx.x] = s;
  }
}

__global__ void __launch_bounds__(TPB) k_head_place(const int32_t *a_d, int R, const int32_t *cnt, int nblk,
                                                    int32_t *rows) {
  __shared__ int red[4][TPB];
  __shared__ int wsum[2][TPB / 64];
  int cb = 0, ct = 0, wb = 0, wt = 0;  // cross / wait rows before this block and in all
  for (int b = threadIdx.x; b < nblk; b += TPB) {
    const int c = cnt[2 * b], w = cnt[2 * b + 1];
    ct += c;
    wt += w;
    if (b < (int)blockIdx.x) cb += c, wb += w;
  }
  red[0][threadIdx.x] = cb;
  red[1][threadIdx.x] = ct;
  red[2][threadIdx.x] = wb;
  red[3][threadIdx.x] = wt;
  __syncthreads();
  for (int st = TPB / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st)
      for (int k = 0; k < 4; k++) red[k][threadIdx.x] += red[k][threadIdx.x + st];
    __syncthreads();
  }
  const int cbase = red[0][0], nc = red[1][0], wbase = red[2][0], nwt = red[3][0];
  const int r = blockIdx.x * TPB + threadIdx.x;
  const bool valid = r < R;
  const bool cross = valid && a_d[r] == 0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t mc = __ballot(cross), mw = __ballot(valid && !cross);
  if (lane == 0) {
    wsum[0][w] = __popcll(mc);
    wsum[1][w] = __popcll(mw);
  }
  __syncthreads();
  int wc = 0, ww = 0;
  for (int q = 0; q < w; q++) wc += wsum[0][q], ww += wsum[1][q];
  const uint64_t lt = lane ? ((1ull << lane) - 1) : 0ull;
  const int ci = cbase + wc + __popcll(mc & lt);  // cross rows before r
  const int wi = wbase + ww + __popcll(mw & lt);  // wait rows before r
  if (valid) rows[cross ? ci : nc + wi] = r;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rows[R] = nc;
    rows[R + 1] = nwt;
  }
}

// The compact record layout (mhppo_rollout_bufs.rec_of): rank[s] = the number of flagged
// segments before s (flag[s] != 0), -1 for an unflagged one.  Two passes as the head lists:
// per-block counts, then every block sums the counts before it and ranks its rows by wave prefix.
__global__ void __launch_bounds__(TPB) k_flag_count(const uint8_t *flag, int R, int32_t *cnt) {
  __shared__ int wsum[TPB / 64];
  const int r = blockIdx.x * TPB + threadIdx.x;
  const uint64_t m = __ballot(r < R && flag[r] != 0);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < TPB / 64; w++) s += wsum[w];
    cnt[blockIdx.x] = s;
  }
}
__global__ void __launch_bounds__(TPB) k_flag_rank(const uint8_t *flag, int R, const int32_t *cnt, int nblk,
                                                   int32_t *rank, int S, int32_t *pre) {
  __shared__ int red[TPB];
  __shared__ int wsum[TPB / 64];
  int before = 0;
  for (int b = threadIdx.x; b < (int)blockIdx.x && b < nblk; b += TPB) before += cnt[b];
  red[threadIdx.x] = before;
  __syncthreads();
  for (int st = TPB / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
    __syncthreads();
  }
  const int r = blockIdx.x * TPB + threadIdx.x;
  const bool f = r < R && flag[r] != 0;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t m = __ballot(f);
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int wc = 0;
  for (int q = 0; q < w; q++) wc += wsum[q];
  const uint64_t below = lane ? (m & ((1ull << lane) - 1)) : 0ull;
  const int nbefore = red[0] + wc + __popcll(below);  // flagged segments before r
  if (r < R) rank[r] = f ? nbefore : -1;
  // pre[g] = flagged segments before segment g S (g = 0 .. R / S): per-group record ranges
  if (r < R && r % S == 0) pre[r / S] = nbefore;
  if (r == R - 1) pre[R / S] = nbefore + (f ? 1 : 0);
}

// Env range of part `part` of `nparts` (the two-stream rollout, RolloutGPU(parts=2)): boundaries at
// multiples of 64 envs (whole waves), the last part ends at N
__host__ __device__ inline int part_env(const Cfg &c, int part, int nparts) {
  if (part >= nparts) return c.N;
  const int64_t b = ((int64_t)part * c.N / nparts + 63) / 64 * 64;
  return (int)std::min<int64_t>(b, c.N);
}

// Per part, where its rows start in the head lists: rows[R + 2 + p] = cross rows of envs before part
// p's first env, rows[R + 2 + nparts + 1 + p] = wait rows likewise (p = 0 .. nparts).  The lists
// are in row order, so a part's rows are one contiguous run of each list (binary search).
__global__ void k_part_bounds(Cfg c, int32_t *rows, int nparts) {
  const int p = threadIdx.x;
  if (p > nparts) return;
  const int R = c.N * c.nS * c.P, nc = rows[R];
  const int rb = part_env(c, p, nparts) * c.nS * c.P;
  int lo = 0, hi = nc;  // first cross index with rows[k] >= rb
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (rows[m] < rb) lo = m + 1;
    else hi = m;
  }
  rows[R + 2 + p] = lo;
  lo = nc, hi = nc + rows[R + 1];  // the wait list
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (rows[m] < rb) lo = m + 1;
    else hi = m;
  }
  rows[R + 2 + nparts + 1 + p] = lo - nc;
}

}  // namespace
