// rollout_record.hip — the collector's bookkeeping between a sampling step and the bucketing, for
// rollouts whose observation rows come from outside the library (+ C-ABI, mhppo_record_begin /
// mhppo_record_step; the contract is include/mhppo.h's).  No env handle: the step's act / logp /
// feat_c are mhppo_policy_sample_act's outputs, rew / rew_light the simulator's.
//
// k_rec_count / k_rec_rank: the compact record layout's ranks (rec_of), rollout_lists.h's
// k_flag_count / k_flag_rank restated on block_prims.h (that header belongs to the rollout.hip
// translation unit and brings the env's device code with it): per-block counts, then every block
// sums the counts before it and ranks its segments by block_rank.  Same block size, same bits.
//
// k_record_step: a block of 256 threads owns 256 consecutive segments.  In the identity layout its
// records are the records [s0, s0 + 256) of step t; in the compact layout the ranks of its present
// segments are consecutive, [R0, R0 + n) with R0 the rank of its first present one (rec_of is a
// prefix count).  Either way the block's output is ONE contiguous run of each array:
//   1. thread j loads its segment's rec_of, act, logp, rew, rew_light and ep_min, takes the
//      episodic minimum, and ranks itself among the block's present segments (block_rank);
//   2. the present segments' three column values go to LDS at their rank; their feature rows are
//      read with adjacent lanes on adjacent floats (a present segment's 52 bytes are contiguous,
//      and so are consecutive present segments'), four loads in flight per lane, into an LDS image
//      of the run;
//   3. every run leaves as 16-byte stores: the image of a run sits in LDS at the run's own offset
//      from a 16-byte boundary (word e of the run at LDS word a + e, a = the destination's word
//      address mod 4), so LDS quad q is destination quad q; the at most two partial quads at the
//      run's ends go out word by word.  float64 values travel as two words.
// All copies move 32-bit words: NaN payloads and signed zeros survive.  No atomics; a block's
// work depends on its index alone.
//
// k_record_step<true> (mhppo_record_step_done) is the same pass with early episode ends: the records
// are stored for every segment, finished or not (the one-contiguous-run-per-block store stays; the
// bucketing never reads a record at or past its stream's length), ep_min is updated only for the
// segments of streams that were running on entry, and the thread of a running stream's slot 0 sets
// len[r] = t + 1 when done[r] != 0.  The S segments of a stream can sit in two blocks, so a thread may
// read len[r] before or after that write.  Liveness rule: a stream is running on entry to step t iff
// len[r] == 0 or len[r] == t + 1.  Steps are recorded once each, in order, so the only value step t
// itself can write is t + 1 and no earlier step can have written it: both reads give the same answer.
#include <hip/hip_runtime.h>

#include "../../include/mhppo.h"
#include "block_prims.h"
#include "common.h"

using namespace mhppo;

namespace {

constexpr int NT = 256;
constexpr int NFC = 13;   // floats of a feature row (obs_car_ped)
constexpr int DEPTH = 4;  // loads in flight per lane in step 2

inline unsigned blocks_for(int64_t n) { return (unsigned)((n + NT - 1) / NT); }

__global__ void __launch_bounds__(NT) k_rec_count(const uint8_t *__restrict__ flag, int R, int32_t *cnt) {
  const int r = blockIdx.x * NT + threadIdx.x;
  const bool f[1] = {r < R && flag[r] != 0};
  int before[1], n[1];
  block_rank<NT>(f, before, n);
  if (threadIdx.x == 0) cnt[blockIdx.x] = n[0];
}

__global__ void __launch_bounds__(NT) k_rec_rank(const uint8_t *__restrict__ flag, int R, const int32_t *cnt, int nblk,
                                                 int32_t *rank, int S, int32_t *pre) {
  int base[1] = {0};  // flagged segments before this block
  for (int b = threadIdx.x; b < (int)blockIdx.x && b < nblk; b += NT) base[0] += cnt[b];
  block_sum<NT>(base);
  const int r = blockIdx.x * NT + threadIdx.x;
  const bool f[1] = {r < R && flag[r] != 0};
  int before[1], n[1];
  block_rank<NT>(f, before, n);
  const int nbefore = base[0] + before[0];  // flagged segments before r
  if (r < R) rank[r] = f[0] ? nbefore : -1;
  // pre[g] = flagged segments before segment g S (g = 0 .. R / S): per-row record ranges
  if (r < R && r % S == 0) pre[r / S] = nbefore;
  if (r == R - 1) pre[R / S] = nbefore + (f[0] ? 1 : 0);
}

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

template <bool DONE>
__global__ void __launch_bounds__(NT)
    k_record_step(int NS, int t, const uint32_t *__restrict__ act, const uint32_t *__restrict__ logp,
                  const uint32_t *__restrict__ feat, const uint2 *__restrict__ rew, const double *__restrict__ rew_light,
                  const int32_t *__restrict__ rec_of, uint32_t *__restrict__ obs_tm, uint32_t *__restrict__ act_tm,
                  uint32_t *__restrict__ logp_tm, uint32_t *__restrict__ rew_tm, double *ep_min, int S,
                  const uint8_t *__restrict__ done, int32_t *len) {
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
    bool live = true;  // the segment's stream was running on entry (the header's liveness rule)
    if (DONE) {
      const int row = s / S;
      const int32_t L = len[row];  // not __restrict__: slot 0's thread of this row may be writing t + 1
      live = L == 0 || L == t + 1;
      if (live && s == row * S && done[row] != 0) len[row] = t + 1;
    }
    if (live) {
      const double m = ep_min[s], x = rew_light[s];
      ep_min[s] = (m != m) ? m : ((x != x) ? x : (x < m ? x : m));  // np.minimum: NaN-propagating
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
int64_t segments(int64_t M, int32_t S) {
  if (M < 0 || S < 1 || M > INT32_MAX / (int64_t)S) return -1;
  return M * S;
}

}  // namespace

extern "C" int64_t mhppo_record_work_bytes(int64_t M, int32_t S) {
  const int64_t NS = segments(M, S);
  if (NS < 0) return set_error(MHPPO_EINVAL, "record_work_bytes: M < 0, S < 1 or M S > 2^31 - 1");
  return ((int64_t)blocks_for(NS) * 4 + 7) / 8 * 8 + 8;
}

extern "C" int mhppo_record_begin(const uint8_t *exist, int64_t M, int32_t S, int32_t *rec_of, double *ep_min,
                                  void *work, void *stream) {
  const int64_t NS = segments(M, S);
  if (NS < 0) return set_error(MHPPO_EINVAL, "record_begin: M < 0, S < 1 or M S > 2^31 - 1");
  if (NS == 0) return MHPPO_OK;
  if (!ep_min) return set_error(MHPPO_EINVAL, "record_begin: ep_min is NULL");
  if (rec_of && (!exist || !work)) return set_error(MHPPO_EINVAL, "record_begin: rec_of needs exist and work");
  hipStream_t st = (hipStream_t)stream;
  CHECK_HIP(hipMemsetAsync(ep_min, 0, (size_t)NS * sizeof(double), st));  // +0.0: np.array([0.]*S) (:383)
  if (rec_of) {
    const unsigned nblk = blocks_for(NS);
    int32_t *cnt = static_cast<int32_t *>(work);
    hipLaunchKernelGGL(k_rec_count, dim3(nblk), dim3(NT), 0, st, exist, (int)NS, cnt);
    hipLaunchKernelGGL(k_rec_rank, dim3(nblk), dim3(NT), 0, st, exist, (int)NS, cnt, (int)nblk, rec_of, (int)S,
                       rec_of + NS);
    CHECK_HIP(hipGetLastError());
  }
  return MHPPO_OK;
}

namespace {
// both entry points: done == NULL is mhppo_record_step
int record_step(const char *who, int64_t M, int32_t S, int32_t t, int32_t T, const float *act, const float *logp,
                const float *feat_c, const double *rew, const double *rew_light, const int32_t *rec_of,
                float *obs_c_tm, float *act_tm, float *logp_tm, double *rew_tm, double *ep_min, bool with_done,
                const uint8_t *done, int32_t *len, void *stream) {
  const int64_t NS = segments(M, S);
  if (NS < 0) return set_error(MHPPO_EINVAL, "%s: M < 0, S < 1 or M S > 2^31 - 1", who);
  if (t < 0 || t >= T) return set_error(MHPPO_EINVAL, "%s: t %d outside [0, %d)", who, t, T);
  if (NS == 0) return MHPPO_OK;
  if (!act || !logp || !feat_c || !rew || !rew_light || !obs_c_tm || !act_tm || !logp_tm || !rew_tm || !ep_min)
    return set_error(MHPPO_EINVAL, "%s: a NULL source or destination", who);
  if (with_done && (!done || !len)) return set_error(MHPPO_EINVAL, "%s: done or len is NULL", who);
  const auto kern = with_done ? k_record_step<true> : k_record_step<false>;
  hipLaunchKernelGGL(kern, dim3(blocks_for(NS)), dim3(NT), 0, (hipStream_t)stream, (int)NS, (int)t,
                     (const uint32_t *)act, (const uint32_t *)logp, (const uint32_t *)feat_c, (const uint2 *)rew,
                     rew_light, rec_of, (uint32_t *)obs_c_tm, (uint32_t *)act_tm, (uint32_t *)logp_tm,
                     (uint32_t *)rew_tm, ep_min, (int)S, done, len);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}
}  // namespace

extern "C" int mhppo_record_step(int64_t M, int32_t S, int32_t t, int32_t T, const float *act, const float *logp,
                                 const float *feat_c, const double *rew, const double *rew_light,
                                 const int32_t *rec_of, float *obs_c_tm, float *act_tm, float *logp_tm,
                                 double *rew_tm, double *ep_min, void *stream) {
  return record_step("record_step", M, S, t, T, act, logp, feat_c, rew, rew_light, rec_of, obs_c_tm, act_tm, logp_tm,
                     rew_tm, ep_min, false, nullptr, nullptr, stream);
}

extern "C" int mhppo_record_step_done(int64_t M, int32_t S, int32_t t, int32_t T, const float *act, const float *logp,
                                      const float *feat_c, const double *rew, const double *rew_light,
                                      const int32_t *rec_of, float *obs_c_tm, float *act_tm, float *logp_tm,
                                      double *rew_tm, double *ep_min, const uint8_t *done, int32_t *len,
                                      void *stream) {
  return record_step("record_step_done", M, S, t, T, act, logp, feat_c, rew, rew_light, rec_of, obs_c_tm, act_tm,
                     logp_tm, rew_tm, ep_min, true, done, len, stream);
}
