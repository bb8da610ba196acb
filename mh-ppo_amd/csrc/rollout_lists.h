// rollout_lists.h — the index lists mhppo_rollout_begin builds once per episode, each by the same
// two passes (per-block counts, then every block sums the counts before it and places its rows by
// their rank in the block; no block waits on another), on the block primitives of block_prims.h:
//   k_head_count / k_head_place   the head lists of k_policy_mfma: the cross rows, then the wait rows
//   k_flag_count / k_flag_rank    the compact record layout's ranks (mhppo_rollout_bufs.rec_of)
//   part_env / k_part_bounds      the env range of a rollout part and where its rows start in the lists
// Part of the rollout.hip translation unit (one anonymous namespace); not for inclusion elsewhere.
#pragma once
#include <algorithm>

#include "block_prims.h"
#include "launch1d.h"
#include "rollout_dev.h"

namespace {
using namespace mhppo;

// Head lists for k_policy_sorted / k_policy_mfma (stable: each list in row order).  Pass 1 counts the
// cross and the wait rows of each 256-row block; pass 2 has every block sum the counts before it
// (and all of them, for the wait list's base), then place its rows by block_rank.
// cnt[2 b] / cnt[2 b + 1]: block b's cross / wait rows.
__global__ void __launch_bounds__(TPB) k_head_count(const int32_t *a_d, int R, int32_t *cnt) {
  const int r = blockIdx.x * TPB + threadIdx.x;
  const bool valid = r < R;
  const bool cross = valid && a_d[r] == 0;  // action_d = 2a - 1 <= 0 (:440-445)
  const bool f[2] = {cross, valid && !cross};
  int before[2], n[2];
  block_rank<TPB>(f, before, n);
  if (threadIdx.x == 0) {
    cnt[2 * blockIdx.x] = n[0];
    cnt[2 * blockIdx.x + 1] = n[1];
  }
}

__global__ void __launch_bounds__(TPB) k_head_place(const int32_t *a_d, int R, const int32_t *cnt, int nblk,
                                                    int32_t *rows) {
  int sum[4] = {0, 0, 0, 0};  // cross rows before this block and in all, wait rows likewise
  for (int b = threadIdx.x; b < nblk; b += TPB) {
    const int c = cnt[2 * b], w = cnt[2 * b + 1];
    sum[1] += c;
    sum[3] += w;
    if (b < (int)blockIdx.x) sum[0] += c, sum[2] += w;
  }
  block_sum<TPB>(sum);
  const int cbase = sum[0], nc = sum[1], wbase = sum[2], nwt = sum[3];
  const int r = blockIdx.x * TPB + threadIdx.x;
  const bool valid = r < R;
  const bool cross = valid && a_d[r] == 0;
  const bool f[2] = {cross, valid && !cross};
  int before[2], n[2];
  block_rank<TPB>(f, before, n);
  const int ci = cbase + before[0];  // cross rows before r
  const int wi = wbase + before[1];  // wait rows before r
  if (valid) rows[cross ? ci : nc + wi] = r;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rows[R] = nc;
    rows[R + 1] = nwt;
  }
}

// The compact record layout (mhppo_rollout_bufs.rec_of): rank[s] = the number of flagged
// segments before s (flag[s] != 0), -1 for an unflagged one.  Two passes as the head lists:
// per-block counts, then every block sums the counts before it and ranks its rows by block_rank.
__global__ void __launch_bounds__(TPB) k_flag_count(const uint8_t *flag, int R, int32_t *cnt) {
  const int r = blockIdx.x * TPB + threadIdx.x;
  const bool f[1] = {r < R && flag[r] != 0};
  int before[1], n[1];
  block_rank<TPB>(f, before, n);
  if (threadIdx.x == 0) cnt[blockIdx.x] = n[0];
}
__global__ void __launch_bounds__(TPB) k_flag_rank(const uint8_t *flag, int R, const int32_t *cnt, int nblk,
                                                   int32_t *rank, int S, int32_t *pre) {
  int base[1] = {0};  // flagged segments before this block
  for (int b = threadIdx.x; b < (int)blockIdx.x && b < nblk; b += TPB) base[0] += cnt[b];
  block_sum<TPB>(base);
  const int r = blockIdx.x * TPB + threadIdx.x;
  const bool f[1] = {r < R && flag[r] != 0};
  int before[1], n[1];
  block_rank<TPB>(f, before, n);
  const int nbefore = base[0] + before[0];  // flagged segments before r
  if (r < R) rank[r] = f[0] ? nbefore : -1;
  // pre[g] = flagged segments before segment g S (g = 0 .. R / S): per-group record ranges
  if (r < R && r % S == 0) pre[r / S] = nbefore;
  if (r == R - 1) pre[R / S] = nbefore + (f[0] ? 1 : 0);
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
