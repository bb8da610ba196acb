// rollout_lanes.hip — auto-reset of external rollouts: several episodes per stream inside one T-step
// window (+ C-ABI, mhppo_lanes_* / mhppo_returns_scan_tm_lanes / mhppo_bucket_scatter_lanes; the contract
// is include/mhppo.h's).  Stream r owns E lanes, lane v = e M + r; the records stay at wall-clock time in
// the identity layout, and a lane is (t0, len) over its stream's columns.
//
// Bookkeeping, one launch each, one thread per element, no loops over the grid:
//   k_lanes_begin    lane 0 of the decision arrays <- the first decision, everything else zero
//   k_lanes_restart  the restarting streams' rows of the fresh decision -> their new lane and the
//                    decision in force.  Whether stream r restarts is read from cur's half of step t - 1
//                    and from len, which this launch does not write; it writes cur's half of step t and
//                    the new lane's t0, which it does not read: no thread reads what another writes.
//   k_record_step<REC_LANES>  record_step.h: the record pass with the current lane's ep_min and end
//   k_lanes_close    len / cut of the batch, into the caller's arrays
// k_returns_tm_lanes: one thread per lane-segment, consecutive threads on consecutive columns of one lane.
// k_scatter_lanes: ppo_batch.hip's ragged scatter with the row of a record looked up per (step, column)
// instead of per column -- a tile of 64 columns x 16 steps can hold pieces of several lanes per column.
// The tile, the LDS layout, the wave butterfly and the partials' order are that kernel's, so the reward
// sums with E == 1 are its bits.
#include <hip/hip_runtime.h>

#include "../../include/mhppo.h"
#include "block_prims.h"
#include "common.h"
#include "record_step.h"

using namespace mhppo;

namespace {

// a decision's arrays as the kernels move them: 32-bit words and exist's bytes
struct Dec {
  uint32_t *a_d, *logp_d, *probs, *feat_d, *closest;
  uint8_t *exist;
};
Dec words(const mhppo_decision &d) {
  return {(uint32_t *)d.a_d, (uint32_t *)d.logp_d, (uint32_t *)d.probs, (uint32_t *)d.feat_d, (uint32_t *)d.closest,
          d.exist};
}
bool complete(const mhppo_decision *d) {
  return d && d->a_d && d->logp_d && d->probs && d->feat_d && d->closest && d->exist;
}
bool complete(const mhppo_lanes *l) { return l && complete(&l->d) && l->ep_min && l->t0 && l->len && l->cur; }

// element idx of an [E][n1] array: lane 0 from src, the other lanes zero
template <typename T>
__device__ __forceinline__ void lane0(T *dst, const T *src, int64_t idx, int64_t n1, int E) {
  if (idx < n1 * E) dst[idx] = idx < n1 ? src[idx] : (T)0;
}

__global__ void __launch_bounds__(NT) k_lanes_begin(Dec L, Dec first, double *ep_min, int32_t *t0, int32_t *len,
                                                    int32_t *cur, int E, int64_t M, int S, int P, int dc) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x, MS = M * S, MSP = MS * P;
  lane0(L.feat_d, first.feat_d, idx, MSP * dc, E);
  lane0(L.probs, first.probs, idx, MSP * 2, E);
  lane0(L.a_d, first.a_d, idx, MSP, E);
  lane0(L.logp_d, first.logp_d, idx, MSP, E);
  lane0(L.closest, first.closest, idx, MS, E);
  lane0(L.exist, first.exist, idx, MS, E);
  if (idx < MS * E) ep_min[idx] = 0.0;  // +0.0, as mhppo_record_begin
  if (idx < M * E) t0[idx] = len[idx] = 0;
  if (idx < 2 * M) cur[idx] = 0;
}

// stream r restarts: its current lane e (on entry) is closed and a lane is left
__device__ __forceinline__ bool restarts(int64_t r, const int32_t *__restrict__ cur_in,
                                         const int32_t *__restrict__ len, int E, int64_t M, int &e) {
  e = cur_in[r];
  return len[(int64_t)e * M + r] != 0 && e + 1 < E;
}

// element idx of an [M][w] array: where its stream restarts, fresh -> the new lane and the decision in force
template <typename T>
__device__ __forceinline__ void merge(T *lanes, T *current, const T *fresh, int64_t idx, int64_t w,
                                      const int32_t *__restrict__ cur_in, const int32_t *__restrict__ len, int E,
                                      int64_t M) {
  if (idx >= M * w) return;
  int e;
  if (!restarts(idx / w, cur_in, len, E, M, e)) return;
  const T x = fresh[idx];
  lanes[(int64_t)(e + 1) * M * w + idx] = x;
  current[idx] = x;
}

__global__ void __launch_bounds__(NT)
    k_lanes_restart(Dec L, Dec fresh, Dec now, int32_t *t0, const int32_t *__restrict__ len,
                    const int32_t *__restrict__ cur_in, int32_t *cur_out, int E, int64_t M, int S, int P, int dc, int t) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x, SP = (int64_t)S * P;
  merge(L.feat_d, now.feat_d, fresh.feat_d, idx, SP * dc, cur_in, len, E, M);
  merge(L.probs, now.probs, fresh.probs, idx, SP * 2, cur_in, len, E, M);
  merge(L.a_d, now.a_d, fresh.a_d, idx, SP, cur_in, len, E, M);
  merge(L.logp_d, now.logp_d, fresh.logp_d, idx, SP, cur_in, len, E, M);
  merge(L.closest, now.closest, fresh.closest, idx, (int64_t)S, cur_in, len, E, M);
  merge(L.exist, now.exist, fresh.exist, idx, (int64_t)S, cur_in, len, E, M);
  if (idx < M) {
    int e;
    const bool go = restarts(idx, cur_in, len, E, M, e);
    cur_out[idx] = e + (go ? 1 : 0);
    if (go) t0[(int64_t)(e + 1) * M + idx] = t;
  }
}

__global__ void __launch_bounds__(NT)
    k_lanes_close(const int32_t *__restrict__ t0, const int32_t *__restrict__ len, const int32_t *__restrict__ cur,
                  int E, int64_t M, int k, int32_t *len_out, uint8_t *cut_out) {
  const int64_t v = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (v >= M * E) return;
  const int64_t e = v / M, r = v - e * M;
  const int32_t L = len[v];
  const bool open = e <= cur[r] && L == 0;  // started and still running
  len_out[v] = open ? k - t0[v] : L;
  cut_out[v] = open ? 1 : 0;
}

__global__ void __launch_bounds__(NT)
    k_returns_tm_lanes(const double *__restrict__ rew, float *__restrict__ ret, int64_t M, int S, int64_t NL, int T,
                       double gamma, const int64_t *__restrict__ pos, const int32_t *__restrict__ t0,
                       const int32_t *__restrict__ len, const uint8_t *__restrict__ cut,
                       const float *__restrict__ v_boot) {
  const int64_t q = (int64_t)blockIdx.x * NT + threadIdx.x;  // lane-segment v S + i
  if (q >= NL || pos[q] < 0) return;
  const int64_t v = q / S, NS = M * S, col = (v % M) * S + (q - v * S);
  const int T0 = min(max(t0[v], 0), T), L = min(max(len[v], 0), T - T0);
  double g = (v_boot && cut[v] != 0 && L > 0) ? (double)v_boot[col] : 0.0;
  for (int t = T0 + L - 1; t >= T0; t--) {
    g = rew[(int64_t)t * NS + col] + gamma * g;
    ret[(int64_t)t * NS + col] = (float)g;
  }
}

namespace lk {
constexpr int SEGS = 64, STEPS = 16, BTPB = SEGS * STEPS;  // one thread per record of the tile
constexpr int OBS_SEG = STEPS * NFC + 1, V_SEG = STEPS + 1;  // LDS strides per column, padded by one word
}
__global__ void __launch_bounds__(lk::BTPB)
    k_scatter_lanes(const int64_t *__restrict__ row0, const int8_t *__restrict__ bucket, const int32_t *__restrict__ t0,
                    const int32_t *__restrict__ len, int64_t NS, int64_t M, int S, int E, int T,
                    const float *__restrict__ obs, const float *__restrict__ act, const float *__restrict__ logp,
                    const float *__restrict__ ret, const double *__restrict__ rew, mhppo_bucket_dst d0,
                    mhppo_bucket_dst d1, double *__restrict__ partials) {
  using namespace lk;
  __shared__ int64_t s_row[SEGS * STEPS];  // the destination row of record (column sg, step tl), -1: none
  __shared__ int8_t s_b[SEGS * STEPS];
  __shared__ float s_obs[SEGS * OBS_SEG];
  __shared__ float s_v[3][SEGS * V_SEG];
  __shared__ double s_rew[SEGS * V_SEG];
  __shared__ double s_sum[2][BTPB / 64];
  const int64_t c0 = (int64_t)blockIdx.x * SEGS;
  const int tb = blockIdx.y * STEPS;
  const int tid = threadIdx.x, sg = tid % SEGS, tl = tid / SEGS;  // a wave is one step of the 64 columns
  const int64_t col = c0 + sg;
  const int t = tb + tl;
  int64_t row = -1;
  int b = 0;
  if (col < NS && t < T) {
    const int64_t r = col / S, i = col - r * S;
    for (int e = 0; e < E; e++) {  // the lane of stream r that holds step t, if any
      const int64_t v = (int64_t)e * M + r, q = v * S + i;
      const int64_t R = row0[q];
      const int j = t - t0[v];
      if (R >= 0 && j >= 0 && j < len[v]) {
        row = R + j;
        b = bucket[q] ? 1 : 0;
        break;
      }
    }
  }
  s_row[sg * STEPS + tl] = row;
  s_b[sg * STEPS + tl] = (int8_t)b;
  __syncthreads();
  {  // one step's observation records of the 64 columns are 64 x 13 consecutive floats
    constexpr int NQ = SEGS * NFC * STEPS / BTPB;
    float v[NQ];
    int at[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int i = tid + q * BTPB, ql = i / (SEGS * NFC), k = i - ql * (SEGS * NFC), qs = k / NFC;
      at[q] = s_row[qs * STEPS + ql] >= 0 ? qs * OBS_SEG + ql * NFC + (k - qs * NFC) : -1;
      v[q] = 0.0f;
      if (at[q] >= 0) v[q] = obs[((int64_t)(tb + ql) * NS + c0) * NFC + k];
    }
#pragma unroll
    for (int q = 0; q < NQ; q++)
      if (at[q] >= 0) s_obs[at[q]] = v[q];
  }
  double acc[2] = {0.0, 0.0};
  if (row >= 0) {
    const int64_t rec = (int64_t)t * NS + col;
    const int o = sg * V_SEG + tl;
    s_v[0][o] = act[rec];
    s_v[1][o] = logp[rec];
    s_v[2][o] = ret[rec];
    const double x = rew[rec];
    s_rew[o] = x;
    acc[b] += (double)(float)x;
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    double a = acc[k];
    for (int m = 32; m > 0; m >>= 1) a += __shfl_xor(a, m, 64);
    if ((tid & 63) == 0) s_sum[k][tid >> 6] = a;
  }
  __syncthreads();
  if (tid < 2) {
    double a = 0.0;
    for (int q = 0; q < BTPB / 64; q++) a += s_sum[tid][q];
    const size_t nblocks = (size_t)gridDim.x * gridDim.y;
    partials[tid * nblocks + (size_t)blockIdx.y * gridDim.x + blockIdx.x] = a;
  }
  // the waves take the columns in turn; consecutive steps of one lane are consecutive rows
  const int w = tid >> 6, l = tid & 63;
  for (int c = w; c < SEGS; c += BTPB / 64) {
    for (int j = l; j < STEPS * NFC; j += 64) {
      const int jl = j / NFC;
      const int64_t R = s_row[c * STEPS + jl];
      if (R >= 0) (s_b[c * STEPS + jl] ? d1 : d0).obs[R * NFC + (j - jl * NFC)] = s_obs[c * OBS_SEG + j];
    }
    if (l < STEPS) {
      const int64_t R = s_row[c * STEPS + l];
      if (R >= 0) {
        const mhppo_bucket_dst &D = s_b[c * STEPS + l] ? d1 : d0;
        const int o = c * V_SEG + l;
        D.act[R] = s_v[0][o];
        D.logp[R] = s_v[1][o];
        D.ret[R] = s_v[2][o];
        D.rew[R] = s_rew[o];
      }
    }
  }
}

constexpr auto k_fold_wide = k_fold<1024, 4, true>;  // mhppo_bucket_scatter_sums' fold

// E M S as the kernels' int, or -1
int64_t lane_segments(int32_t E, int64_t M, int32_t S) {
  const int64_t NS = segments(M, S);
  if (E < 1 || NS < 0 || NS > INT32_MAX / (int64_t)E) return -1;
  return NS * E;
}

// the grid of a one-thread-per-element launch over n elements, or 0: too many
unsigned grid_of(int64_t n) {
  const int64_t nb = (n + NT - 1) / NT;
  return nb > INT32_MAX ? 0u : (unsigned)nb;
}

}  // namespace

extern "C" int mhppo_lanes_begin(const mhppo_lanes *lanes, int32_t E, int64_t M, int32_t S, int32_t P, int32_t dc,
                                 const mhppo_decision *first, void *stream) {
  const int64_t NL = lane_segments(E, M, S);
  if (NL < 0 || P < 1 || dc < 1) return set_error(MHPPO_EINVAL, "lanes_begin: E < 1, M < 0, S < 1, E M S > 2^31 - 1, P < 1 or dc < 1");
  if (M == 0) return MHPPO_OK;
  if (!complete(lanes) || !complete(first)) return set_error(MHPPO_EINVAL, "lanes_begin: a NULL pointer");
  const unsigned g = grid_of(NL * P * (dc > 2 ? dc : 2));
  if (!g) return set_error(MHPPO_EINVAL, "lanes_begin: E M S P dc is too large for one launch");
  hipLaunchKernelGGL(k_lanes_begin, dim3(g), dim3(NT), 0, (hipStream_t)stream, words(lanes->d), words(*first),
                     lanes->ep_min, lanes->t0, lanes->len, lanes->cur, (int)E, M, (int)S, (int)P, (int)dc);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

extern "C" int mhppo_lanes_restart(const mhppo_lanes *lanes, int32_t E, int64_t M, int32_t S, int32_t P, int32_t dc,
                                   int32_t t, int32_t T, const mhppo_decision *fresh, const mhppo_decision *current,
                                   void *stream) {
  const int64_t NL = lane_segments(E, M, S);
  if (NL < 0 || P < 1 || dc < 1) return set_error(MHPPO_EINVAL, "lanes_restart: E < 1, M < 0, S < 1, E M S > 2^31 - 1, P < 1 or dc < 1");
  if (t < 1 || t >= T) return set_error(MHPPO_EINVAL, "lanes_restart: t %d outside [1, %d)", t, T);
  if (M == 0) return MHPPO_OK;
  if (!complete(lanes) || !complete(fresh) || !complete(current))
    return set_error(MHPPO_EINVAL, "lanes_restart: a NULL pointer");
  const unsigned g = grid_of(M * S * P * (dc > 2 ? dc : 2));
  if (!g) return set_error(MHPPO_EINVAL, "lanes_restart: M S P dc is too large for one launch");
  int32_t *cur = lanes->cur;
  hipLaunchKernelGGL(k_lanes_restart, dim3(g), dim3(NT), 0, (hipStream_t)stream, words(lanes->d), words(*fresh),
                     words(*current), lanes->t0, lanes->len, cur + (size_t)((t - 1) & 1) * M, cur + (size_t)(t & 1) * M,
                     (int)E, M, (int)S, (int)P, (int)dc, (int)t);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

extern "C" int mhppo_lanes_record(const mhppo_lanes *lanes, int32_t E, int64_t M, int32_t S, int32_t t, int32_t T,
                                  const float *act, const float *logp, const float *feat_c, const double *rew,
                                  const double *rew_light, float *obs_c_tm, float *act_tm, float *logp_tm,
                                  double *rew_tm, const uint8_t *done, void *stream) {
  if (lane_segments(E, M, S) < 0) return set_error(MHPPO_EINVAL, "lanes_record: E < 1, M < 0, S < 1 or E M S > 2^31 - 1");
  if (t < 0 || t >= T) return set_error(MHPPO_EINVAL, "lanes_record: t %d outside [0, %d)", t, T);
  if (M == 0) return MHPPO_OK;
  if (!complete(lanes) || !act || !logp || !feat_c || !rew || !rew_light || !obs_c_tm || !act_tm || !logp_tm ||
      !rew_tm || !done)
    return set_error(MHPPO_EINVAL, "lanes_record: a NULL pointer");
  const int64_t NS = M * S;
  hipLaunchKernelGGL(k_record_step<REC_LANES>, dim3(blocks_for(NS)), dim3(NT), 0, (hipStream_t)stream, (int)NS, (int)t,
                     (const uint32_t *)act, (const uint32_t *)logp, (const uint32_t *)feat_c, (const uint2 *)rew,
                     rew_light, (const int32_t *)nullptr, (uint32_t *)obs_c_tm, (uint32_t *)act_tm,
                     (uint32_t *)logp_tm, (uint32_t *)rew_tm, lanes->ep_min, (int)S, done, lanes->len,
                     (const int32_t *)(lanes->cur + (size_t)(t & 1) * M), (const int32_t *)lanes->t0, (int)M);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

extern "C" int mhppo_lanes_close(const mhppo_lanes *lanes, int32_t E, int64_t M, int32_t k, int32_t T,
                                 int32_t *len_out, uint8_t *cut_out, void *stream) {
  if (E < 1 || M < 0 || M > INT32_MAX / (int64_t)E) return set_error(MHPPO_EINVAL, "lanes_close: E < 1, M < 0 or E M > 2^31 - 1");
  if (k < 1 || k > T) return set_error(MHPPO_EINVAL, "lanes_close: k %d outside [1, %d]", k, T);
  if (M == 0) return MHPPO_OK;
  if (!lanes || !lanes->t0 || !lanes->len || !lanes->cur || !len_out || !cut_out)
    return set_error(MHPPO_EINVAL, "lanes_close: a NULL pointer");
  hipLaunchKernelGGL(k_lanes_close, dim3(blocks_for(M * E)), dim3(NT), 0, (hipStream_t)stream, lanes->t0, lanes->len,
                     lanes->cur + (size_t)((k - 1) & 1) * M, (int)E, M, (int)k, len_out, cut_out);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

extern "C" int mhppo_returns_scan_tm_lanes(const double *rew, float *ret, int64_t M, int32_t S, int32_t E, int32_t T,
                                           double gamma, const int64_t *pos, const int32_t *t0, const int32_t *len,
                                           const uint8_t *cut, const float *v_boot, void *stream) {
  const int64_t NL = lane_segments(E, M, S);
  if (NL < 0 || T < 1) return set_error(MHPPO_EINVAL, "returns_scan_tm_lanes: E < 1, M < 0, S < 1, E M S > 2^31 - 1 or T < 1");
  if (M == 0) return MHPPO_OK;
  if (!rew || !ret || !pos || !t0 || !len || !cut) return set_error(MHPPO_EINVAL, "returns_scan_tm_lanes: a NULL pointer");
  hipStream_t s = (hipStream_t)stream;
  CHECK_HIP(hipMemsetAsync(ret, 0, (size_t)T * M * S * sizeof(float), s));
  hipLaunchKernelGGL(k_returns_tm_lanes, dim3(blocks_for(NL)), dim3(NT), 0, s, rew, ret, M, (int)S, NL, (int)T, gamma,
                     pos, t0, len, cut, v_boot);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

extern "C" int mhppo_bucket_scatter_lanes(const int64_t *row0, const int8_t *bucket, const int32_t *t0,
                                          const int32_t *len, int64_t M, int32_t S, int32_t E, int32_t T,
                                          const float *obs_tm, const float *act_tm, const float *logp_tm,
                                          const float *ret_tm, const double *rew_tm, const mhppo_bucket_dst *dst,
                                          double *rew_sums, void *work, void *stream) {
  if (lane_segments(E, M, S) < 0 || T < 1 || !dst)
    return set_error(MHPPO_EINVAL, "bucket_scatter_lanes: E < 1, M < 0, S < 1, E M S > 2^31 - 1, T < 1 or dst NULL");
  if (M == 0) return MHPPO_OK;
  if (!row0 || !bucket || !t0 || !len || !obs_tm || !act_tm || !logp_tm || !ret_tm || !rew_tm || !rew_sums || !work)
    return set_error(MHPPO_EINVAL, "bucket_scatter_lanes: a NULL pointer");
  const int64_t NS = M * S;
  dim3 g((unsigned)((NS + lk::SEGS - 1) / lk::SEGS), (unsigned)((T + lk::STEPS - 1) / lk::STEPS));
  const int64_t nblocks = (int64_t)g.x * g.y;
  if (nblocks > INT32_MAX) return set_error(MHPPO_EINVAL, "bucket_scatter_lanes: too many records");
  hipStream_t s = (hipStream_t)stream;
  double *part = (double *)work;
  hipLaunchKernelGGL(k_scatter_lanes, g, dim3(lk::BTPB), 0, s, row0, bucket, t0, len, NS, M, (int)S, (int)E, (int)T,
                     obs_tm, act_tm, logp_tm, ret_tm, rew_tm, dst[0], dst[1], part);
  hipLaunchKernelGGL(k_fold_wide, dim3(2), dim3(1024), 0, s, part, (int)nblocks, rew_sums);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}
