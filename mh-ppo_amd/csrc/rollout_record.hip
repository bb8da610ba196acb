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
// k_record_step (record_step.h, shared with rollout_lanes.hip): a block of 256 threads owns 256
// consecutive segments.  In the identity layout its records are the records [s0, s0 + 256) of
// step t; in the compact layout the ranks of its present
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
// k_record_step<REC_DONE> (mhppo_record_step_done) is the same pass with early episode ends: the records
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
#include "record_step.h"

using namespace mhppo;

namespace {

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
  const auto kern = with_done ? k_record_step<REC_DONE> : k_record_step<REC_PLAIN>;
  hipLaunchKernelGGL(kern, dim3(blocks_for(NS)), dim3(NT), 0, (hipStream_t)stream, (int)NS, (int)t,
                     (const uint32_t *)act, (const uint32_t *)logp, (const uint32_t *)feat_c, (const uint2 *)rew,
                     rew_light, rec_of, (uint32_t *)obs_c_tm, (uint32_t *)act_tm, (uint32_t *)logp_tm,
                     (uint32_t *)rew_tm, ep_min, (int)S, done, len, (const int32_t *)nullptr,
                     (const int32_t *)nullptr, 0);
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
