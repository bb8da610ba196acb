// ppo_batch.hip — from a finished rollout's time-major records to the update's batches (+ C-ABI):
//   k_returns / k_returns_tm / k_returns_tm_len   the reward-to-go scan (mhppo_returns_scan / _scan_tm /
//                              _scan_tm_len: a length per column)
//   k_returns_tm_boot          the same scan started from a bootstrap value per column
//                              (mhppo_returns_scan_tm_boot)
//   k_bucket_scatter           both segment-major buckets in one pass over the records, optionally
//                              with their reward sums, folded by k_fold<1024, 4, add>
//                              (mhppo_bucket_scatter / _scatter_sums; RAGGED: _scatter_ragged)
//   k_rag_count / _scan / _place    the ragged buckets' row offsets and lengths (mhppo_ragged_plan;
//                              scratch size: mhppo_ragged_work_bytes)
//   k_plan_count / _scan / _place   the bucket positions, the choice batch and the host's one info
//                              record (mhppo_bucket_plan; scratch size: mhppo_bucket_work_bytes)
// Every sum has a fixed order (block_prims.h: the fold and the ballot rank): the same call gives
// the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/mhppo.h"
#include "block_prims.h"
#include "common.h"
#include "launch1d.h"
#include "ppo_math.h"  // NF_C

using namespace mhppo;

namespace {

// ------------------------------------------------------------ returns
// futur_rewards (:668-672): episodic_reward = rew + 0.99*episodic_reward, float64,
// then torch.tensor(..., dtype=float) -> float32
__global__ void __launch_bounds__(TPB) k_returns(const double *rew, float *ret, int64_t B, int T, double gamma) {
  int64_t b = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (b >= B) return;
  const double *r = rew + b * T;
  float *o = ret + b * T;
  double g = 0.0;
  for (int t = T - 1; t >= 0; t--) {
    g = r[t] + gamma * g;
    o[t] = (float)g;
  }
}

// time-major records [T][B]: lane b scans column b (coalesced across the wave)
__global__ void __launch_bounds__(TPB) k_returns_tm(const double *rew, float *ret, int64_t B, int T, double gamma) {
  int64_t b = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (b >= B) return;
  double g = 0.0;
  for (int t = T - 1; t >= 0; t--) {
    g = rew[(int64_t)t * B + b] + gamma * g;
    ret[(int64_t)t * B + b] = (float)g;
  }
}

// the same scan of a column cut at len_rec[b] steps (clamped to [0, T]; NULL: T): G starts from 0 at
// t = len - 1 (the early end is terminal, as the time limit is) and ret is 0 from there on
__global__ void __launch_bounds__(TPB)
    k_returns_tm_len(const double *rew, float *ret, int64_t B, int T, double gamma, const int32_t *len_rec) {
  int64_t b = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (b >= B) return;
  const int L = len_rec ? min(max(len_rec[b], 0), T) : T;
  for (int t = T - 1; t >= L; t--) ret[(int64_t)t * B + b] = 0.0f;
  double g = 0.0;
  for (int t = L - 1; t >= 0; t--) {
    g = rew[(int64_t)t * B + b] + gamma * g;
    ret[(int64_t)t * B + b] = (float)g;
  }
}

// k_returns_tm_len started from G = v_boot[b] instead of 0 at t = L - 1 (a truncated segment's V(s_L);
// L == 0: v_boot is not read).  Nothing else differs.
__global__ void __launch_bounds__(TPB) k_returns_tm_boot(const double *rew, float *ret, int64_t B, int T, double gamma,
                                                         const int32_t *len_rec, const float *v_boot) {
  int64_t b = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (b >= B) return;
  const int L = len_rec ? min(max(len_rec[b], 0), T) : T;
  for (int t = T - 1; t >= L; t--) ret[(int64_t)t * B + b] = 0.0f;
  double g = L > 0 ? (double)v_boot[b] : 0.0;
  for (int t = L - 1; t >= 0; t--) {
    g = rew[(int64_t)t * B + b] + gamma * g;
    ret[(int64_t)t * B + b] = (float)g;
  }
}

// ------------------------------------------------------------ bucket scatter
// Segment-major buckets (bucket_segments; the reference's per-episode concatenation,
// Coop-MH-PPO-scalable.py:489-507), both buckets in one pass over the time-major records:
// record (t, s) of a segment s in bucket b = bucket[s] (pos[s] >= 0) goes to row pos[s]*T + t
// of bucket b.  A block owns 64 segments x 16 steps: coalesced loads of the records (64
// consecutive segments per step) into LDS, then each segment's 16 rows leave as contiguous
// runs — every record read once and every bucket row written once, in full lines.
namespace bk {
constexpr int SEGS = 64, STEPS = 16;
// LDS strides per segment, padded by one word: phase 1 writes one step of 64 consecutive
// segments per instruction, and unpadded strides (208 / 16 words) put those 64 lanes on 4
// banks (16-way conflicts on every record field)
constexpr int OBS_SEG = STEPS * NF_C + 1, V_SEG = STEPS + 1;
#ifndef MHPPO_BK_TPB
#define MHPPO_BK_TPB 1024  // 16 waves: two blocks (75 KB of LDS each) fill a CU
#endif
constexpr int BTPB = MHPPO_BK_TPB;
}
// SUMS (mhppo_bucket_scatter_sums): partials[b * nblocks + block] = the block's sum of
// (double)(float)rew over its records of bucket b (wave butterflies, then the waves in order: a
// fixed order), folded by k_fold_wide.
// RAGGED (mhppo_bucket_scatter_ragged): pos[s] is the segment's first ROW (row0) instead of its
// position, and only its first len_rec[s] steps are records: the tile's step count is per segment,
// ns = clamp(len_rec[s] - t0, 0, nt), its rows row0 + t0 .. + ns.  Nothing at or past a length is
// loaded, summed or written.
template <bool SUMS, bool RAGGED>
__global__ void __launch_bounds__(bk::BTPB)
    k_bucket_scatter(const int64_t *__restrict__ pos, const int8_t *__restrict__ bucket, int64_t NS, int T,
                     const float *__restrict__ obs, const float *__restrict__ act, const float *__restrict__ logp,
                     const float *__restrict__ ret, const double *__restrict__ rew, mhppo_bucket_dst d0,
                     mhppo_bucket_dst d1, double *__restrict__ partials, const int32_t *__restrict__ len_rec) {
  using namespace bk;
  __shared__ int s_ns[RAGGED ? SEGS : 1];  // RAGGED: the segments' step counts in this tile
  __shared__ float s_obs[SEGS * OBS_SEG];
  __shared__ float s_v[3][SEGS * V_SEG];
  __shared__ double s_rew[SEGS * V_SEG];
  __shared__ int64_t s_pos[SEGS];
  __shared__ int8_t s_b[SEGS];
  __shared__ double s_sum[2][SUMS ? BTPB / 64 : 1];
  const int64_t s0 = (int64_t)blockIdx.x * SEGS;
  const int t0 = blockIdx.y * STEPS;
  const int nseg = (int)min((int64_t)SEGS, NS - s0), nt = min(STEPS, T - t0);
  const int tid = threadIdx.x;
  if (tid < SEGS) {
    s_pos[tid] = tid < nseg ? pos[s0 + tid] : -1;
    s_b[tid] = tid < nseg ? bucket[s0 + tid] : 0;
    if (RAGGED) s_ns[tid] = tid < nseg ? min(max(len_rec[s0 + tid] - t0, 0), nt) : 0;
  }
  __syncthreads();
  // the observation records of one step of the block's 64 segments are 64 x 13 consecutive
  // floats: lanes read them as one flat run (every load instruction on two 128-byte lines), all
  // of a lane's loads issued before its first LDS store.  Only records of bucketed segments are
  // loaded (exec-masked): the scalable env's non-existent slots (pos < 0) cost no fetch unless a
  // bucketed neighbour shares their 128-byte line.
  {
    constexpr int NQ = SEGS * NF_C * STEPS / BTPB;
    static_assert(SEGS * NF_C * STEPS % BTPB == 0, "bucket scatter: block size");
    float v[NQ];
    int at[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int i = tid + q * BTPB, tl = i / (SEGS * NF_C), k = i - tl * (SEGS * NF_C), sg = k / NF_C;
      const bool in = sg < nseg && tl < (RAGGED ? s_ns[sg] : nt);
      at[q] = in && s_pos[sg] >= 0 ? sg * OBS_SEG + tl * NF_C + (k - sg * NF_C) : -1;
      v[q] = 0.0f;
      if (at[q] >= 0) v[q] = obs[((int64_t)(t0 + tl) * NS + s0) * NF_C + k];
    }
#pragma unroll
    for (int q = 0; q < NQ; q++)
      if (at[q] >= 0) s_obs[at[q]] = v[q];
  }
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int i = tid; i < SEGS * STEPS; i += BTPB) {  // i = step * SEGS + seg: lanes on consecutive segments
    const int sg = i % SEGS, tl = i / SEGS;
    if (sg >= nseg || tl >= (RAGGED ? s_ns[sg] : nt) || s_pos[sg] < 0) continue;
    const int64_t rec = (int64_t)(t0 + tl) * NS + s0 + sg;
    const int o = sg * V_SEG + tl;  // LDS: segment-major
    s_v[0][o] = act[rec];
    s_v[1][o] = logp[rec];
    s_v[2][o] = ret[rec];
    const double r = rew[rec];
    s_rew[o] = r;
    if (SUMS) acc[s_b[sg] ? 1 : 0] += (double)(float)r;
  }
  if (SUMS) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      double a = acc[k];
      for (int m = 32; m > 0; m >>= 1) a += __shfl_xor(a, m, 64);
      if ((tid & 63) == 0) s_sum[k][tid >> 6] = a;
    }
  }
  __syncthreads();
  if (SUMS && tid < 2) {
    double a = 0.0;
    for (int q = 0; q < BTPB / 64; q++) a += s_sum[tid][q];
    const size_t nblocks = (size_t)gridDim.x * gridDim.y;
    partials[tid * nblocks + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = a;
  }
  // the waves take the segments in turn: segment sg's rows pos*T + t0 .. + nt leave as one run
  const int w = tid >> 6, l = tid & 63;
  for (int sg = w; sg < nseg; sg += BTPB / 64) {
    const int64_t p = s_pos[sg];
    if (p < 0) continue;
    const mhppo_bucket_dst &D = s_b[sg] ? d1 : d0;
    const int64_t r0 = RAGGED ? p + t0 : p * T + t0;
    const int ns = RAGGED ? s_ns[sg] : nt;
    float *oo = D.obs + r0 * NF_C;
    for (int j = l; j < ns * NF_C; j += 64) oo[j] = s_obs[sg * OBS_SEG + j];
    if (l < ns) {
      const int o = sg * V_SEG + l;
      D.act[r0 + l] = s_v[0][o];
      D.logp[r0 + l] = s_v[1][o];
      D.ret[r0 + l] = s_v[2][o];
      D.rew[r0 + l] = s_rew[o];
    }
  }
}

// ------------------------------------------------------------ bucket plan
// mhppo_bucket_plan: what bucket_segments needs before its one host read, in three launches (no
// block waits on another): per-block counts (k_plan_count), ONE block scans them and writes the
// mhppo_bucket_info record (k_plan_scan), then every block places its segments by their rank in
// the block (k_plan_place; block_prims.h block_rank).
struct PlanSeg {
  int64_t base;  // the segment's choice row: s P + closest[s]
  int a_car;     // a_d there (the choice batch's action)
  bool exist, cross, wait;
};
__device__ inline PlanSeg plan_seg(int64_t s, int S, int P, const int32_t *__restrict__ a_d,
                                   const int32_t *__restrict__ closest, const uint8_t *__restrict__ exist, int fix) {
  PlanSeg q;
  const int cl = min(max(closest[s], 0), P - 1);
  q.base = s * P + cl;
  q.a_car = a_d[q.base];
  // the reference's bucket rule reads action_d[i], the per-(car, ped) array at the CAR index i
  // (SURVEY Q13); fix: the car's closest pedestrian's decision.  Cross when 2 a - 1 <= 0.
  const int64_t n = s / S;
  const int a = fix ? q.a_car : a_d[n * S * P + (s - n * S)];
  q.exist = exist[s] != 0;
  q.cross = q.exist && a <= 0;
  q.wait = q.exist && a > 0;
  return q;
}

constexpr int PLAN_NC = 5;  // per-block counts: cross, wait, existing, existing with a_car == 0 / == 1

__global__ void __launch_bounds__(TPB)
    k_plan_count(int64_t NS, int S, int P, const int32_t *__restrict__ a_d, const int32_t *__restrict__ closest,
                 const uint8_t *__restrict__ exist, const double *__restrict__ ep_min, int fix, int nblk,
                 int32_t *__restrict__ cnt, double *__restrict__ epart, int64_t *__restrict__ pos,
                 int8_t *__restrict__ bucket) {
  const int64_t s = (int64_t)blockIdx.x * TPB + threadIdx.x;
  bool f[PLAN_NC] = {false, false, false, false, false};
  double e[1] = {0.0};
  if (s < NS) {
    const PlanSeg q = plan_seg(s, S, P, a_d, closest, exist, fix);
    f[0] = q.cross, f[1] = q.wait, f[2] = q.exist;
    f[3] = q.exist && q.a_car == 0, f[4] = q.exist && q.a_car == 1;
    if (q.exist) e[0] = (double)(float)ep_min[s];  // the choice batch's reward (float32), summed in float64
    pos[s] = -1;  // k_plan_place fills in the bucketed segments (records, in the compact layout)
    bucket[s] = 0;
  }
  int before[PLAN_NC], c[PLAN_NC];
  block_rank<TPB>(f, before, c);
  block_sum<TPB>(e);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < PLAN_NC; k++) cnt[(size_t)k * nblk + blockIdx.x] = c[k];
    epart[blockIdx.x] = e[0];
  }
}

// one block: base[k][b] = the sum of cnt[k][0 .. b) for k = cross, wait, existing (tiles of TPB
// blocks, a running carry between tiles), the totals and the info record
__global__ void __launch_bounds__(TPB)
    k_plan_scan(const int32_t *__restrict__ cnt, const double *__restrict__ epart, int nblk,
                const int32_t *__restrict__ status, int32_t *__restrict__ base, mhppo_bucket_info *__restrict__ info) {
  __shared__ int wsum[TPB / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int64_t total[PLAN_NC];
#pragma unroll
  for (int k = 0; k < PLAN_NC; k++) {
    int64_t carry = 0;
    for (int b0 = 0; b0 < nblk; b0 += TPB) {
      const int b = b0 + tid;
      const int v = b < nblk ? cnt[(size_t)k * nblk + b] : 0;
      int x = v;  // inclusive scan over the wave, then over the waves
      for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
      }
      if (lane == 63) wsum[w] = x;
      __syncthreads();
      int before = 0, all = 0;
      for (int q = 0; q < TPB / 64; q++) {
        if (q < w) before += wsum[q];
        all += wsum[q];
      }
      if (k < 3 && b < nblk) base[(size_t)k * nblk + b] = (int32_t)(carry + before + x - v);
      carry += all;
      __syncthreads();
    }
    total[k] = carry;
  }
  double e[1] = {strided_sum<TPB, 1>(epart, nblk)};  // the fold's order: one chain, TPB threads
  block_sum<TPB>(e);
  if (tid == 0) {
    info->n_cross = total[0];
    info->n_wait = total[1];
    info->n_all = total[2];
    info->status = status ? status[0] : 0;
    info->counts[0] = (double)total[3];
    info->counts[1] = (double)total[4];
    info->rew_sums[0] = 0.0;  // the scatter's fold adds the cross / wait sums
    info->rew_sums[1] = 0.0;
    info->rew_sums[2] = e[0];
  }
}

__global__ void __launch_bounds__(TPB)
    k_plan_place(int64_t NS, int S, int P, int dc, const int32_t *__restrict__ a_d,
                 const int32_t *__restrict__ closest, const uint8_t *__restrict__ exist,
                 const int32_t *__restrict__ rec_of, const double *__restrict__ ep_min,
                 const float *__restrict__ feat_d, const float *__restrict__ logp_d, int fix, int nblk,
                 const int32_t *__restrict__ base, const mhppo_bucket_info *__restrict__ info,
                 int64_t *__restrict__ pos, int8_t *__restrict__ bucket, float *__restrict__ c_obs,
                 int32_t *__restrict__ c_act, float *__restrict__ c_logp, float *__restrict__ c_ret) {
  __shared__ int64_t s_src[TPB];
  const int tid = threadIdx.x;
  const int64_t s = (int64_t)blockIdx.x * TPB + tid;
  PlanSeg q;
  q.base = 0, q.a_car = 0, q.exist = q.cross = q.wait = false;
  if (s < NS) q = plan_seg(s, S, P, a_d, closest, exist, fix);
  const bool f[3] = {q.cross, q.wait, q.exist};
  int before[3], total[3];
  block_rank<TPB>(f, before, total);
  const int64_t ci = (int64_t)base[blockIdx.x] + before[0];                 // cross segments before s
  const int64_t wi = (int64_t)base[(size_t)nblk + blockIdx.x] + before[1];  // wait segments before s
  const int er = before[2], ne = total[2];  // existing segments before s in this block, and in all of it
  const int64_t eb = base[2 * (size_t)nblk + blockIdx.x];
  // the wait bucket starts at the cross count rounded up to a multiple of 4 (bucket_segments)
  const int64_t w0 = (info->n_cross + 3) / 4 * 4;
  if (q.cross || q.wait) {
    int64_t r = s;  // the compact layout: positions are per record
    if (rec_of) r = rec_of[s];
    if (r >= 0 && r < NS) {
      pos[r] = q.cross ? ci : w0 + wi;
      bucket[r] = q.cross ? 0 : 1;
    }
  }
  // the choice batch, existing segments first in (env, slot) order: the block's rows are the
  // contiguous run [eb, eb + ne); the features leave as one flat coalesced copy
  if (q.exist) {
    s_src[er] = q.base;
    c_act[eb + er] = q.a_car;
    c_logp[eb + er] = logp_d[q.base];
    c_ret[eb + er] = (float)ep_min[s];
  }
  __syncthreads();
  float *o = c_obs + eb * dc;
  for (int i = tid; i < ne * dc; i += TPB) {
    const int r = i / dc, c = i - r * dc;
    o[i] = feat_d[s_src[r] * dc + c];
  }
}

// ------------------------------------------------------------ ragged plan
// mhppo_ragged_plan: the buckets' row offsets when the streams have lengths of their own, in the
// bucket plan's three-launch shape (no block waits on another, no atomics): per-block sums of the
// lengths (k_rag_count), ONE block scans them and writes info (k_rag_scan), then every block places
// its segments by the exclusive sum of the lengths before them in the block (k_rag_place).
// A thread owns SEGMENT s, whose record column is b = s (identity) or rec_of[s] (compact).  The sums
// run in segment order; row0 is defined in column order.  The two agree because rec_of ascends with
// s (mhppo_record_begin's ranks), and the rows then follow the order of pos because
// mhppo_bucket_plan ranks the columns of a bucket in column order.
struct RagSeg {
  int64_t col;  // the segment's record column, -1: none
  int len;      // the effective length of its stream
  bool in0, in1;
};
__device__ inline RagSeg rag_seg(int64_t s, int64_t NS, int S, int k, const int64_t *__restrict__ pos,
                                 const int8_t *__restrict__ bucket, const int32_t *__restrict__ rec_of,
                                 const int32_t *__restrict__ len) {
  RagSeg q;
  q.col = -1, q.len = 0, q.in0 = q.in1 = false;
  if (s >= NS) return q;
  const int64_t b = rec_of ? (int64_t)rec_of[s] : s;
  if (b < 0 || b >= NS) return q;
  const int32_t L = len[s / S];
  q.col = b;
  q.len = (L <= 0 || L > k) ? k : L;  // 0: still running, cut at k
  const bool used = pos[b] >= 0;
  q.in1 = used && bucket[b] != 0;
  q.in0 = used && !q.in1;
  return q;
}

// v[k] <- the sum of v[k] over the threads before this one in the block, total[k] <- over all of it
// (inclusive shuffle scan per wave, then the waves in order).  Called by every thread.
__device__ __forceinline__ void block_excl_scan2(int64_t (&v)[2], int64_t (&total)[2]) {
  __shared__ int64_t wsum[2][TPB / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int64_t own = v[k];
    int64_t x = own;
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (lane == 63) wsum[k][w] = x;
    v[k] = x - own;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; k++) {
    int64_t before = 0, all = 0;
    for (int q = 0; q < TPB / 64; q++) {
      if (q < w) before += wsum[k][q];
      all += wsum[k][q];
    }
    v[k] += before;
    total[k] = all;
  }
  __syncthreads();  // wsum may be written again
}

__global__ void __launch_bounds__(TPB)
    k_rag_count(int64_t NS, int S, int k, const int64_t *__restrict__ pos, const int8_t *__restrict__ bucket,
                const int32_t *__restrict__ rec_of, const int32_t *__restrict__ len, int nblk,
                int64_t *__restrict__ sums, int64_t *__restrict__ row0, int32_t *__restrict__ len_rec) {
  const int64_t s = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const RagSeg q = rag_seg(s, NS, S, k, pos, bucket, rec_of, len);
  if (s < NS) {  // as a COLUMN index: k_rag_place fills in the columns that hold a record
    row0[s] = -1;
    len_rec[s] = 0;
  }
  int64_t v[2] = {q.in0 ? q.len : 0, q.in1 ? q.len : 0}, total[2];
  block_excl_scan2(v, total);
  if (threadIdx.x == 0) {
    sums[blockIdx.x] = total[0];
    sums[(size_t)nblk + blockIdx.x] = total[1];
  }
}

// one block: base[k][b] = the sum of sums[k][0 .. b) (tiles of TPB blocks, a running carry), info = the totals
__global__ void __launch_bounds__(TPB)
    k_rag_scan(const int64_t *__restrict__ sums, int nblk, int64_t *__restrict__ base, int64_t *__restrict__ info) {
  int64_t carry[2] = {0, 0};
  for (int b0 = 0; b0 < nblk; b0 += TPB) {
    const int b = b0 + threadIdx.x;
    int64_t v[2] = {b < nblk ? sums[b] : 0, b < nblk ? sums[(size_t)nblk + b] : 0}, total[2];
    block_excl_scan2(v, total);
    if (b < nblk) {
      base[b] = carry[0] + v[0];
      base[(size_t)nblk + b] = carry[1] + v[1];
    }
    carry[0] += total[0];
    carry[1] += total[1];
  }
  if (threadIdx.x == 0) {
    info[0] = carry[0];  // rows_cross
    info[1] = carry[1];  // rows_wait
  }
}

__global__ void __launch_bounds__(TPB)
    k_rag_place(int64_t NS, int S, int k, const int64_t *__restrict__ pos, const int8_t *__restrict__ bucket,
                const int32_t *__restrict__ rec_of, const int32_t *__restrict__ len, int nblk,
                const int64_t *__restrict__ base, const int64_t *__restrict__ info, int64_t *__restrict__ row0,
                int32_t *__restrict__ len_rec) {
  const int64_t s = (int64_t)blockIdx.x * TPB + threadIdx.x;
  const RagSeg q = rag_seg(s, NS, S, k, pos, bucket, rec_of, len);
  int64_t v[2] = {q.in0 ? q.len : 0, q.in1 ? q.len : 0}, total[2];
  block_excl_scan2(v, total);
  if (q.col < 0) return;
  len_rec[q.col] = q.len;
  // the wait rows start at the cross rows rounded up to a multiple of 4 (16-byte aligned 52-byte rows)
  const int64_t w0 = (info[0] + 3) / 4 * 4;
  if (q.in0) row0[q.col] = base[blockIdx.x] + v[0];
  if (q.in1) row0[q.col] = w0 + base[(size_t)nblk + blockIdx.x] + v[1];
}

// the fold of the scatter's partials (two per block: many), added to rew_sums
constexpr int FOLD_TPB = 1024;
constexpr auto k_fold_wide = k_fold<FOLD_TPB, 4, true>;

}  // namespace

extern "C" {

int mhppo_returns_scan(const double *rew, float *ret, int64_t B, int32_t T, double gamma, void *stream) {
  if (!rew || !ret || B < 0 || T <= 0) return set_error(MHPPO_EINVAL, "bad argument");
  if (B == 0) return MHPPO_OK;
  hipLaunchKernelGGL(k_returns, grid_for(B), dim3(TPB), 0, (hipStream_t)stream, rew, ret, B, T, gamma);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_returns_scan_tm(const double *rew, float *ret, int64_t B, int32_t T, double gamma, void *stream) {
  if (!rew || !ret || B < 0 || T <= 0) return set_error(MHPPO_EINVAL, "bad argument");
  if (B == 0) return MHPPO_OK;
  hipLaunchKernelGGL(k_returns_tm, grid_for(B), dim3(TPB), 0, (hipStream_t)stream, rew, ret, B, T, gamma);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_bucket_scatter(const int64_t *pos, const int8_t *bucket, int64_t NS, int32_t T, const float *obs_tm,
                         const float *act_tm, const float *logp_tm, const float *ret_tm, const double *rew_tm,
                         const mhppo_bucket_dst *dst, void *stream) {
  if (NS < 0 || T <= 0 || !dst) return set_error(MHPPO_EINVAL, "bad argument");
  if (NS == 0) return MHPPO_OK;
  if (!pos || !bucket || !obs_tm || !act_tm || !logp_tm || !ret_tm || !rew_tm)
    return set_error(MHPPO_EINVAL, "null pointer");
  const int64_t nb = (NS + bk::SEGS - 1) / bk::SEGS;
  if (nb > 0x7fffffff) return set_error(MHPPO_EINVAL, "too many segments");
  dim3 g((unsigned)nb, (unsigned)((T + bk::STEPS - 1) / bk::STEPS));
  hipLaunchKernelGGL((k_bucket_scatter<false, false>), g, dim3(bk::BTPB), 0, (hipStream_t)stream, pos, bucket, NS,
                     (int)T, obs_tm, act_tm, logp_tm, ret_tm, rew_tm, dst[0], dst[1], (double *)nullptr,
                     (const int32_t *)nullptr);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

// scratch of the bucket plan (per-block counts, their scans, the ep_min partials) and of the
// scatter's reward sums (two partials per block); the two calls run in stream order and may share it
static int64_t plan_blocks(int64_t NS) { return (NS + TPB - 1) / TPB; }
static int64_t scatter_blocks(int64_t NS, int32_t T) {
  return ((NS + bk::SEGS - 1) / bk::SEGS) * ((T + bk::STEPS - 1) / bk::STEPS);
}
int64_t mhppo_bucket_work_bytes(int64_t NS, int32_t T) {
  if (NS < 0 || T < 0) return 0;
  const int64_t plan = plan_blocks(NS) * (8 + 4 * (PLAN_NC + 3)) + 8, sc = scatter_blocks(NS, T) * 16;
  return std::max<int64_t>(std::max(plan, sc), 8);
}

int mhppo_bucket_scatter_sums(const int64_t *pos, const int8_t *bucket, int64_t NS, int32_t T, const float *obs_tm,
                              const float *act_tm, const float *logp_tm, const float *ret_tm, const double *rew_tm,
                              const mhppo_bucket_dst *dst, double *rew_sums, void *work, void *stream) {
  if (NS < 0 || T <= 0 || !dst) return set_error(MHPPO_EINVAL, "bad argument");
  if (NS == 0) return MHPPO_OK;
  if (!pos || !bucket || !obs_tm || !act_tm || !logp_tm || !ret_tm || !rew_tm || !rew_sums || !work)
    return set_error(MHPPO_EINVAL, "null pointer");
  const int64_t nb = (NS + bk::SEGS - 1) / bk::SEGS, nblocks = scatter_blocks(NS, T);
  if (nb > 0x7fffffff || nblocks > 0x7fffffff) return set_error(MHPPO_EINVAL, "too many segments");
  dim3 g((unsigned)nb, (unsigned)((T + bk::STEPS - 1) / bk::STEPS));
  hipStream_t s = (hipStream_t)stream;
  double *part = (double *)work;
  hipLaunchKernelGGL((k_bucket_scatter<true, false>), g, dim3(bk::BTPB), 0, s, pos, bucket, NS, (int)T, obs_tm, act_tm,
                     logp_tm, ret_tm, rew_tm, dst[0], dst[1], part, (const int32_t *)nullptr);
  hipLaunchKernelGGL(k_fold_wide, dim3(2), dim3(FOLD_TPB), 0, s, part, (int)nblocks, rew_sums);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_bucket_plan(int64_t N, int32_t S, int32_t P, int32_t dc, const int32_t *a_d, const int32_t *closest,
                      const uint8_t *exist, const int32_t *rec_of, const double *ep_min, const float *feat_d,
                      const float *logp_d, int32_t fix_bucket, const int32_t *status, int64_t *pos, int8_t *bucket,
                      float *c_obs, int32_t *c_act, float *c_logp, float *c_ret, mhppo_bucket_info *info,
                      void *work, void *stream) {
  if (N < 0 || S <= 0 || P <= 0 || dc <= 0) return set_error(MHPPO_EINVAL, "bad argument");
  if (!info || !work) return set_error(MHPPO_EINVAL, "null pointer");
  const int64_t NS = N * S;
  if (NS * P > 0x7fffffff) return set_error(MHPPO_EINVAL, "too many segments");
  if (NS > 0 && (!a_d || !closest || !exist || !ep_min || !feat_d || !logp_d || !pos || !bucket || !c_obs || !c_act ||
                 !c_logp || !c_ret))
    return set_error(MHPPO_EINVAL, "null pointer");
  const int nblk = (int)plan_blocks(NS);
  // work: epart double [nblk] | cnt int32 [PLAN_NC][nblk] | base int32 [3][nblk]
  double *epart = (double *)work;
  int32_t *cnt = (int32_t *)(epart + nblk), *base = cnt + (size_t)PLAN_NC * nblk;
  hipStream_t s = (hipStream_t)stream;
  if (nblk > 0)
    hipLaunchKernelGGL(k_plan_count, dim3(nblk), dim3(TPB), 0, s, NS, (int)S, (int)P, a_d, closest, exist, ep_min,
                       (int)fix_bucket, nblk, cnt, epart, pos, bucket);
  hipLaunchKernelGGL(k_plan_scan, dim3(1), dim3(TPB), 0, s, cnt, epart, nblk, status, base, info);
  if (nblk > 0)
    hipLaunchKernelGGL(k_plan_place, dim3(nblk), dim3(TPB), 0, s, NS, (int)S, (int)P, (int)dc, a_d, closest, exist,
                       rec_of, ep_min, feat_d, logp_d, (int)fix_bucket, nblk, base, info, pos, bucket, c_obs, c_act,
                       c_logp, c_ret);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_returns_scan_tm_len(const double *rew, float *ret, int64_t B, int32_t T, double gamma,
                              const int32_t *len_rec, void *stream) {
  if (!rew || !ret || B < 0 || T <= 0) return set_error(MHPPO_EINVAL, "returns_scan_tm_len: bad argument");
  if (B == 0) return MHPPO_OK;
  hipLaunchKernelGGL(k_returns_tm_len, grid_for(B), dim3(TPB), 0, (hipStream_t)stream, rew, ret, B, T, gamma, len_rec);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_returns_scan_tm_boot(const double *rew, float *ret, int64_t B, int32_t T, double gamma,
                               const int32_t *len_rec, const float *v_boot, void *stream) {
  if (!v_boot) return mhppo_returns_scan_tm_len(rew, ret, B, T, gamma, len_rec, stream);
  if (!rew || !ret || B < 0 || T <= 0) return set_error(MHPPO_EINVAL, "returns_scan_tm_boot: bad argument");
  if (B == 0) return MHPPO_OK;
  hipLaunchKernelGGL(k_returns_tm_boot, grid_for(B), dim3(TPB), 0, (hipStream_t)stream, rew, ret, B, T, gamma, len_rec,
                     v_boot);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

// scratch of the ragged plan: the per-block length sums and their scans, int64 [2][nblk] each
int64_t mhppo_ragged_work_bytes(int64_t NS) {
  if (NS < 0) return 0;
  return std::max<int64_t>(plan_blocks(NS) * 32, 8);
}

int mhppo_ragged_plan(const int64_t *pos, const int8_t *bucket, const int32_t *rec_of, const int32_t *len, int64_t M,
                      int32_t S, int32_t k, int64_t *row0, int32_t *len_rec, int64_t *info, void *work,
                      void *stream) {
  if (M < 0 || S < 1 || M > INT32_MAX / (int64_t)S) return set_error(MHPPO_EINVAL, "ragged_plan: M < 0, S < 1 or M S > 2^31 - 1");
  if (k < 1) return set_error(MHPPO_EINVAL, "ragged_plan: k < 1");
  if (!info || !work) return set_error(MHPPO_EINVAL, "ragged_plan: info or work is NULL");
  const int64_t NS = M * S;
  if (NS > 0 && (!pos || !bucket || !len || !row0 || !len_rec))
    return set_error(MHPPO_EINVAL, "ragged_plan: a NULL pointer other than rec_of");
  const int nblk = (int)plan_blocks(NS);
  int64_t *sums = (int64_t *)work, *base = sums + 2 * (size_t)nblk;
  hipStream_t s = (hipStream_t)stream;
  if (nblk > 0)
    hipLaunchKernelGGL(k_rag_count, dim3(nblk), dim3(TPB), 0, s, NS, (int)S, (int)k, pos, bucket, rec_of, len, nblk, sums,
                       row0, len_rec);
  hipLaunchKernelGGL(k_rag_scan, dim3(1), dim3(TPB), 0, s, sums, nblk, base, info);
  if (nblk > 0)
    hipLaunchKernelGGL(k_rag_place, dim3(nblk), dim3(TPB), 0, s, NS, (int)S, (int)k, pos, bucket, rec_of, len, nblk, base,
                       info, row0, len_rec);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_bucket_scatter_ragged(const int64_t *row0, const int8_t *bucket, const int32_t *len_rec, int64_t NS,
                                int32_t T, const float *obs_tm, const float *act_tm, const float *logp_tm,
                                const float *ret_tm, const double *rew_tm, const mhppo_bucket_dst *dst,
                                double *rew_sums, void *work, void *stream) {
  if (NS < 0 || T <= 0 || !dst) return set_error(MHPPO_EINVAL, "bucket_scatter_ragged: bad argument");
  if (NS == 0) return MHPPO_OK;
  if (!row0 || !bucket || !len_rec || !obs_tm || !act_tm || !logp_tm || !ret_tm || !rew_tm || !rew_sums || !work)
    return set_error(MHPPO_EINVAL, "bucket_scatter_ragged: null pointer");
  const int64_t nb = (NS + bk::SEGS - 1) / bk::SEGS, nblocks = scatter_blocks(NS, T);
  if (nb > 0x7fffffff || nblocks > 0x7fffffff) return set_error(MHPPO_EINVAL, "bucket_scatter_ragged: too many segments");
  dim3 g((unsigned)nb, (unsigned)((T + bk::STEPS - 1) / bk::STEPS));
  hipStream_t s = (hipStream_t)stream;
  double *part = (double *)work;
  hipLaunchKernelGGL((k_bucket_scatter<true, true>), g, dim3(bk::BTPB), 0, s, row0, bucket, NS, (int)T, obs_tm, act_tm,
                     logp_tm, ret_tm, rew_tm, dst[0], dst[1], part, len_rec);
  hipLaunchKernelGGL(k_fold_wide, dim3(2), dim3(FOLD_TPB), 0, s, part, (int)nblocks, rew_sums);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

}  // extern "C"
