// record_step.h — k_record_step, the one-contiguous-run-per-block store of a step's records, for the
// two units that launch it: rollout_record.hip (mhppo_record_step, mhppo_record_step_done) and
// rollout_lanes.hip (mhppo_lanes_record).  The pass is described in rollout_record.hip's header; MODE
// selects what happens beside the stores:
//   REC_PLAIN  ep_min of every segment
//   REC_DONE   early episode ends: ep_min of the running streams' segments, len[r] = t + 1 on a done
//   REC_LANES  auto-reset lanes (identity layout): stream r's current lane is e = cur[r], lane
//              v = e M + r; the lane runs on entry to step t iff len[v] == 0 or len[v] == t + 1 - t0[v]
//              (REC_DONE's liveness rule per lane: the only value this step can write, and no earlier
//              step can have written it); ep_min is the lanes' [E, NS] array, updated at e NS + s
//              for running lanes; slot 0's thread closes the lane on done.  cur, t0 and len of other
//              lanes are not written by this launch.
// For those two units only: NT, NFC, blocks_for and segments are short names in an anonymous namespace,
// chosen for the record pass; no other unit should include this header.
#pragma once
#include <hip/hip_runtime.h>

#include "block_prims.h"

namespace {

constexpr int NT = 256;
constexpr int NFC = 13;   // floats of a feature row (obs_car_ped)
constexpr int DEPTH = 4;  // loads in flight per lane in step 2
constexpr int REC_PLAIN = 0, REC_DONE = 1, REC_LANES = 2;

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + NT - 1) / NT); }

// Word offset of p from the 16-byte boundary below it (p is 4-byte aligned).
__device__ __forceinline__ int quad_off(const void *p) { return (int)(((uintptr_t)p >> 2) & 3); }

// The run dst[0 .. C) <- img[a .. a + C), a = quad_off(dst), img 16-byte aligned in LDS: whole quads
// as 16-byte stores, the partial ones at the ends word by word.  Called by the whole block.
__device__ __forceinline__ void store_run(uint32_t *__restrict__ dst, const uint32_t *img, int a, int C) {
  uint4 *d4 = reinterpret_cast<uint4 *>(dst - a);  // 16-byte aligned; quads outside the run are not touched
  const uint4 *s4 = reinterpret_cast<const uint4 *>(img);
  const int end = a + C, nq = (end + 3) >> 2;
  for (int q = threadIdx.x; q < nq; q += NT) {
    const int lo = 4 * q;
    if (lo >= a && lo + 4 <= end) {
      d4[q] = s4[q];
    } else {
#pragma unroll
      for (int w = lo; w < lo + 4; w++)
        if (w >= a && w < end) dst[w - a] = img[w];
    }
  }
}

template <int MODE>
__global__ void __launch_bounds__(NT)
    k_record_step(int NS, int t, const uint32_t *__restrict__ act, const uint32_t *__restrict__ logp,
                  const uint32_t *__restrict__ feat, const uint2 *__restrict__ rew, const double *__restrict__ rew_light,
                  const int32_t *__restrict__ rec_of, uint32_t *__restrict__ obs_tm, uint32_t *__restrict__ act_tm,
                  uint32_t *__restrict__ logp_tm, uint32_t *__restrict__ rew_tm, double *ep_min, int S,
                  const uint8_t *__restrict__ done, int32_t *len, const int32_t *__restrict__ cur,
                  const int32_t *__restrict__ t0, int M) {
  // LDS images of the block's runs, each with room for its offset a <= 3 from a 16-byte boundary
  __shared__ uint4 img_o[(NT * NFC + 3 + 3) / 4];
  __shared__ uint4 img_a[(NT + 3 + 3) / 4], img_l[(NT + 3 + 3) / 4], img_r[(2 * NT + 3 + 3) / 4];
  __shared__ int src[NT];  // the block's present segments, in order (thread indices)
  __shared__ int first;    // the record of the block's first present segment
  const int j = threadIdx.x;
  const int s0 = blockIdx.x * NT;  // < NS <= 2^31 - 1
  const int nvalid = NS - s0 < NT ? NS - s0 : NT;
  const bool valid = j < nvalid;
  const int s = s0 + j;
  int r = -1;
  uint32_t va = 0, vl = 0;
  uint2 vr = make_uint2(0, 0);
  if (valid) {
    r = rec_of ? rec_of[s] : s;
    va = act[s];
    vl = logp[s];
    vr = rew[s];
    bool live = true;        // the segment's stream was running on entry (the header's liveness rule)
    int64_t m_at = s;        // the segment's ep_min
    if (MODE == REC_DONE) {
      const int row = s / S;
      const int32_t L = len[row];  // not __restrict__: slot 0's thread of this row may be writing t + 1
      live = L == 0 || L == t + 1;
      if (live && s == row * S && done[row] != 0) len[row] = t + 1;
    }
    if (MODE == REC_LANES) {
      const int row = s / S;
      const int e = cur[row];
      const int64_t v = (int64_t)e * M + row;
      const int32_t L = len[v], here = t + 1 - t0[v];  // len: slot 0's thread of this row may be writing `here`
      live = L == 0 || L == here;
      if (live && s == row * S && done[row] != 0) len[v] = here;
      m_at = (int64_t)e * NS + s;
    }
    if (live) {
      const double m = ep_min[m_at], x = rew_light[s];
      ep_min[m_at] = (m != m) ? m : ((x != x) ? x : (x < m ? x : m));  // np.minimum: NaN-propagating
    }
  }
  const bool f[1] = {r >= 0};
  int before[1], total[1];
  block_rank<NT>(f, before, total);
  const int n = total[0], k = before[0];
  if (f[0]) {
    src[k] = j;
    if (k == 0) first = r;
  }
  __syncthreads();
  if (n == 0) return;
  const int R0 = first;
  if (R0 < 0 || (int64_t)R0 + n > NS) return;  // not a rec_of of mhppo_record_begin: nothing out of bounds
  const int64_t rec0 = (int64_t)t * NS + R0;   // the run's first record of step t
  uint32_t *d_o = obs_tm + rec0 * NFC, *d_a = act_tm + rec0, *d_l = logp_tm + rec0, *d_r = rew_tm + rec0 * 2;
  const int a_o = quad_off(d_o), a_a = quad_off(d_a), a_l = quad_off(d_l), a_r = quad_off(d_r);
  uint32_t *io = reinterpret_cast<uint32_t *>(img_o), *ia = reinterpret_cast<uint32_t *>(img_a);
  uint32_t *il = reinterpret_cast<uint32_t *>(img_l), *ir = reinterpret_cast<uint32_t *>(img_r);
  if (f[0]) {
    ia[a_a + k] = va;
    il[a_l + k] = vl;
    ir[a_r + 2 * k] = vr.x;
    ir[a_r + 2 * k + 1] = vr.y;
  }
  const int ne = n * NFC;
  const uint32_t *fsrc = feat + (int64_t)s0 * NFC;
  for (int e0 = j; e0 < ne; e0 += DEPTH * NT) {
    uint32_t v[DEPTH];
#pragma unroll
    for (int u = 0; u < DEPTH; u++) {
      const int e = e0 + u * NT;
      if (e < ne) {
        const int row = e / NFC;
        v[u] = fsrc[src[row] * NFC + (e - row * NFC)];
      }
    }
#pragma unroll
    for (int u = 0; u < DEPTH; u++)
      if (e0 + u * NT < ne) io[a_o + e0 + u * NT] = v[u];
  }
  __syncthreads();
  store_run(d_o, io, a_o, ne);
  store_run(d_a, ia, a_a, n);
  store_run(d_l, il, a_l, n);
  store_run(d_r, ir, a_r, 2 * n);
}

// M S as the kernels' int, or -1
inline int64_t segments(int64_t M, int32_t S) {
  if (M < 0 || S < 1 || M > INT32_MAX / (int64_t)S) return -1;
  return M * S;
}

}  // namespace
