// rollout.hip — the GPU rollout collector and the deterministic evaluation step (+ C-ABI).
//
// Per episode (Env_rollout.iterations_rand, Coop-MH-PPO-scalable.py:357-517), for N envs at once:
//   begin:  env reset -> choice features -> choice actor -> Categorical draw (k_choice, below), then
//           the head lists and, in the compact record layout, the record ranks (rollout_lists.h)
//   step t: [k_policy_mfma] per (env, slot, ped) row: obs_car_ped features and the
//           cross/wait actor picked by action_d (head-sorted 32-row f32-MFMA tiles);
//           [k_sample_env] one lane per env: min over pedestrians, MVN draw,
//           log-prob, rollout-buffer writes, then the env step itself (the same
//           env_step_one the standalone step kernel runs) and the episodic min.
// This file holds the host side (argument checks, the choice of kernel, the launches, the
// dispatch-attached kernel timing, the debug exports of the A/B builds) and k_choice.  The other
// kernels are in the headers below, all in this TU's anonymous namespace; this is the only unit
// that compiles the env step (env_body.h).  What follows a rollout — returns, buckets, losses —
// is in ppo_batch.hip and ppo_loss.hip, the noise in noise.hip.
//   rollout_policy.h   the policy step: k_policy_mfma (and the test build's VALU references)
//   rollout_lists.h    the head lists, the record ranks, the part bounds
//   rollout_step.h     k_sample_env[_r], k_eval_step, k_fill_f64
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <vector>

#include <algorithm>
#include <math.h>
#include <string.h>

#include "../../include/mhppo.h"
#include "common.h"
#include "env_body.h"
#include "launch1d.h"
#include "ppo_heads.h"
#include "rollout_dev.h"
#include "rollout_policy.h"
#include "rollout_lists.h"
#include "rollout_step.h"

using namespace mhppo;

namespace mhppo {
const Cfg &env_cfg(const mhppo_env *env);
const Bufs &env_bufs(const mhppo_env *env);
int env_device(const mhppo_env *env);
}  // namespace mhppo

namespace {
// -------------------------------------------------------------- begin
// one lane per (env, slot, ped): choice features, choice actor, Categorical draw.
// LDS: the observation rows of the block's envs (one flat coalesced copy:
// a lane's features read its env's row from LDS, not one strided global load per feature), then the
// block's feature rows (row-per-lane, stride dc + 1: conflict-free), written to feat_d as ONE flat
// coalesced run of TPB x dc floats after the forward (which reads its inputs from that LDS row).
// Before: each lane stored its dc-float row straight to global memory at a dc-float stride and the
// forward read it back from there — 8.6x (cfg3) / 17x (cfg4) the algorithmic HBM traffic.
__host__ __device__ inline int choice_env_span(const Cfg &c) {  // envs a TPB-row block can touch
  return (TPB + c.nS * c.P - 1) / (c.nS * c.P) + 1;
}
// (The actor's weights are wave-uniform: read through the scalar cache as SGPR operands of the
// fmaf chains — W is a separate __restrict__ argument, so the compiler may use scalar loads — not
// staged in LDS, where every weight cost the LDS pipe a read per lane-group.)
__host__ __device__ inline size_t choice_lds_floats(const Cfg &c) {
  return (size_t)choice_env_span(c) * c.obs_dim + (size_t)TPB * (choice_dim(c) + 1);
}
template <int V>
__global__ void __launch_bounds__(TPB)
    k_choice(Cfg c, const float *__restrict__ W, const float *u, const int32_t *forced, mhppo_rollout_bufs B) {
  extern __shared__ float lds[];
  const ObsLayout L = obs_layout(c);
  const int dc = choice_dim(c), SP = c.nS * c.P, od = L.obs_dim;
  const size_t R = (size_t)c.N * SP, r0 = (size_t)blockIdx.x * TPB;
  const int nr = (int)min((size_t)TPB, R - r0);
  float *s_obs = lds, *s_f = s_obs + (size_t)choice_env_span(c) * od;
  const size_t e0 = r0 / SP, e1 = (r0 + nr - 1) / SP;  // the block's envs [e0, e1]
  const int nobs = (int)(e1 - e0 + 1) * od;
  for (int i = threadIdx.x; i < nobs; i += TPB) s_obs[i] = B.obs[e0 * od + i];
  __syncthreads();
  const int t = threadIdx.x;
  const size_t r = r0 + t;
  const int fs = dc + 1;  // LDS feature-row stride (odd: conflict-free row-per-lane access)
  float *f = s_f + (size_t)t * fs;
  if (t < nr) {
    const int p = (int)(r % c.P), i = (int)((r / c.P) % c.nS);
    const size_t e = r / SP;
    const float *o = s_obs + (e - e0) * od;
    obs_car_ped_d(o, L, i, p, f);
    if (p == 0) {
      B.closest[e * c.nS + i] = closest_ped_d(o, L, i);
      B.exist[e * c.nS + i] = L.scalable ? (uint8_t)(o[i * L.cw + 6] != 0.0f) : (uint8_t)1;
    }
    float pr[2];
    // the scalable 8-slot head (dc 54) and the coop / 4cars 4-slot one (27) fully unrolled
    if (dc == 54) mlp_forward_rows<54, 2>(W, f, pr);
    else if (dc == 27) mlp_forward_rows<27, 2>(W, f, pr);
    else mlp_forward<0, 2>(W, dc, f, pr);
    float p0, p1, n[2];
    softmax_pair<LibmRollout>(pr[0], pr[1], p0, p1);  // Model_PPO type 2 (:81-85)
    reinterpret_cast<float2 *>(B.probs_d)[r] = make_float2(p0, p1);
    if ((p0 != p0 || p1 != p1) && B.status) atomicOr(B.status, 1u);  // Categorical raises on NaN probs
    // Categorical(probs): normalise, clamp to [eps, 1-eps], log (torch/distributions/utils.py)
    cat_normalise(p0, p1, n);
    int a = forced ? forced[r] : (u[r] >= n[0] ? 1 : 0);
    B.a_d[r] = a;
    B.logp_d[r] = logf(cat_clamp(a ? n[1] : n[0]));
  }
  __syncthreads();
  // the block's feature rows [r0, r0 + nr) x dc: one contiguous run of floats
  float *dst = B.feat_d + r0 * dc;
  for (int k = t; k < nr * dc; k += TPB) dst[k] = s_f[(k / dc) * fs + k % dc];
}

// -------------------------------------------------------------- host side
#define VLAUNCH(kern, variant, grid, shm, stream, ...) VLAUNCHB(kern, variant, grid, dim3(TPB), shm, stream, __VA_ARGS__)
#define VLAUNCHB(kern, variant, grid, block, shm, stream, ...)                                               \
  do {                                                                                                       \
    switch (variant) {                                                                                       \
      case V_COOP: hipLaunchKernelGGL(kern<V_COOP>, grid, block, shm, stream, __VA_ARGS__); break;           \
      case V_4CARS: hipLaunchKernelGGL(kern<V_4CARS>, grid, block, shm, stream, __VA_ARGS__); break;         \
      case V_SCALABLE: hipLaunchKernelGGL(kern<V_SCALABLE>, grid, block, shm, stream, __VA_ARGS__); break;   \
      case V_NAIF: hipLaunchKernelGGL(kern<V_NAIF>, grid, block, shm, stream, __VA_ARGS__); break;           \
      case V_STOP: hipLaunchKernelGGL(kern<V_STOP>, grid, block, shm, stream, __VA_ARGS__); break;           \
      default:                                                                                               \
        return set_error(MHPPO_EINVAL, "the rollout/evaluation drivers do not support variant %d (4cars2: "    \
                         "the reference has no driver and its followers earn no reward)", variant);          \
    }                                                                                                        \
  } while (0)

// Dispatch-attached timing of the env-step launches (mhppo_kernel_timing_begin/_end): the
// next n launches of the calling thread on the device current at _begin record a start/stop
// pair with their dispatch.  The events belong to that device (recreated when _begin runs on
// another one) and are reused across begin/end pairs (2 * the largest n, per thread).
struct KernelTiming {
  std::vector<hipEvent_t> ev;  // [2 * cap]
  int cap = 0, used = 0, dev = -1;
  bool on = false;
};
thread_local KernelTiming g_ktime;
inline bool ktime_next(hipEvent_t &a, hipEvent_t &b) {
  KernelTiming &k = g_ktime;
  if (!k.on || k.used >= k.cap) return false;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != k.dev) return false;  // a launch on another device: untimed
  a = k.ev[2 * k.used];
  b = k.ev[2 * k.used + 1];
  k.used++;
  return true;
}

// register-view rollout step for a compiled shape (4cars2 has no rollout driver)
template <int V, int NC, int NAV, int NP>
bool launch_sample_reg(const Cfg &c, const Bufs &eb, const float *eps, int t, const mhppo_rollout_bufs &B,
                       hipStream_t s, int e_lo, int e_hi) {
  if constexpr (V == V_4CARS2) {
    return false;
  } else {
    if (!use_reg_view(c, V, NC, NAV, NP)) return false;
    const dim3 g = grid_for((size_t)(e_hi - e_lo));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (ktime_next(e0, e1))  // same launch, with the timing events attached to its dispatch
      hipExtLaunchKernelGGL((k_sample_env_r<V, NC, NAV, NP>), g, dim3(TPB), 0, s, e0, e1, 0, c, eb, eps, t, B, e_lo,
                            e_hi);
    else
      hipLaunchKernelGGL((k_sample_env_r<V, NC, NAV, NP>), g, dim3(TPB), 0, s, c, eb, eps, t, B, e_lo, e_hi);
    return true;
  }
}

}  // namespace

extern "C" {

#ifdef MHPPO_WAVE_TIMES
int mhppo_debug_wave_times(unsigned long long *out) {  // [2 * 8192]: start, end per wave
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_times), sizeof(unsigned long long) * 2 * 8192));
  return MHPPO_OK;
}
#endif
#ifdef MHPPO_TIMING
// A/B timing builds only (not part of include/mhppo.h): copy out and clear g_timing
int mhppo_debug_timing(unsigned long long *out16) {
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_timing), sizeof(unsigned long long) * 16));
  unsigned long long z[32] = {0};
  CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_timing), z, sizeof(z)));
  return MHPPO_OK;
}
// the per-phase slowest-wave cycles (g_timing[16 + k]); read before mhppo_debug_timing clears them
int mhppo_debug_timing_max(unsigned long long *out16) {
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_timing), sizeof(unsigned long long) * 16,
                                sizeof(unsigned long long) * 16));
  return MHPPO_OK;
}
#endif

int mhppo_choice_dim(const mhppo_env *env) { return env ? choice_dim(env_cfg(env)) : MHPPO_EINVAL; }

int mhppo_rollout_begin(mhppo_env *env, const mhppo_mlp *actor_choice, const float *u, const int32_t *forced_a,
                        mhppo_rollout_bufs *bufs, void *stream) {
  if (!env || !actor_choice || !bufs || (!u && !forced_a)) return set_error(MHPPO_EINVAL, "null argument");
  if (bufs->parts < 0 || bufs->parts > 63) return set_error(MHPPO_EINVAL, "parts %d outside [0, 63]", bufs->parts);
  if (bufs->parts > 1 && !bufs->rows) return set_error(MHPPO_EINVAL, "parts > 1 needs the head lists (rows)");
  GUARD_DEVICE(env_device(env));
  const Cfg &c = env_cfg(env);
  if (actor_choice->n_in != choice_dim(c) || actor_choice->n_out != 2)
    return set_error(MHPPO_EINVAL, "choice actor must be %d -> 2 (got %d -> %d)", choice_dim(c), actor_choice->n_in,
                     actor_choice->n_out);
  hipStream_t s = (hipStream_t)stream;
  // the NaN flags cover this episode only (a flag left by an unchecked earlier collect must not
  // surface at a later, clean iteration's mhppo_rollout_check)
  if (bufs->status) CHECK_HIP(hipMemsetAsync(bufs->status, 0, sizeof(uint32_t), s));
  int rc = mhppo_env_reset(env, bufs->obs, stream);
  if (rc) return rc;
  size_t R = (size_t)c.N * c.nS * c.P;
  size_t shm = sizeof(float) * choice_lds_floats(c);
  if (shm > 160 * 1024) return set_error(MHPPO_EINVAL, "choice kernel LDS %zu B (obs_dim %d, dc %d)", shm, c.obs_dim, choice_dim(c));
  VLAUNCH(k_choice, c.variant, grid_for(R), shm, s, c, actor_choice->packed, u, forced_a, *bufs);
  size_t NS = (size_t)c.N * c.nS;
  if (bufs->rec_of) {  // the compact record layout: present segments ranked in (env, slot) order
    if (c.variant != V_SCALABLE) return set_error(MHPPO_EINVAL, "rec_of: the scalable env's layout only");
    if (!bufs->exist) return set_error(MHPPO_EINVAL, "rec_of needs exist");
    const int nblk = (int)grid_for(NS).x;
    int32_t *cnt = reinterpret_cast<int32_t *>(scratch((nblk + 1) / 2));
    if (!cnt) return set_error(MHPPO_ENOMEM, "scratch allocation failed");
    hipLaunchKernelGGL(k_flag_count, grid_for(NS), dim3(TPB), 0, s, bufs->exist, (int)NS, cnt);
    hipLaunchKernelGGL(k_flag_rank, grid_for(NS), dim3(TPB), 0, s, bufs->exist, (int)NS, cnt, nblk, bufs->rec_of,
                       c.nS, bufs->rec_of + NS);
  }
  if (bufs->rows) {  // head lists for k_policy_mfma (the choice is fixed for the episode)
    const int nblk = (int)grid_for(R).x;
    int32_t *cnt = reinterpret_cast<int32_t *>(scratch(nblk));
    if (!cnt) return set_error(MHPPO_ENOMEM, "scratch allocation failed");
    // every row: a car slot absent at t = 0 (no record) can be present later in the episode, and its
    // action then drives the env (skipping those rows diverged the scalable reference rollout)
    hipLaunchKernelGGL(k_head_count, grid_for(R), dim3(TPB), 0, s, bufs->a_d, (int)R, cnt);
    hipLaunchKernelGGL(k_head_place, grid_for(R), dim3(TPB), 0, s, bufs->a_d, (int)R, cnt, nblk, bufs->rows);
    if (bufs->parts > 1) hipLaunchKernelGGL(k_part_bounds, dim3(1), dim3(64), 0, s, c, bufs->rows, (int)bufs->parts);
  }
  hipLaunchKernelGGL(k_fill_f64, grid_for(NS), dim3(TPB), 0, s, bufs->ep_min, NS, 0.0);  // np.array([0.]*S) (:383)
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

static int rollout_policy(mhppo_env *env, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                          mhppo_rollout_bufs *bufs, int part, int nparts, void *stream);

int mhppo_rollout_policy(mhppo_env *env, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                         mhppo_rollout_bufs *bufs, void *stream) {
  return rollout_policy(env, actor_cross, actor_wait, bufs, 0, 1, stream);
}

int mhppo_rollout_policy_part(mhppo_env *env, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                              mhppo_rollout_bufs *bufs, int part, void *stream) {
  if (!bufs) return set_error(MHPPO_EINVAL, "null argument");
  const int np = bufs->parts > 1 ? bufs->parts : 1;
  if (part < 0 || part >= np) return set_error(MHPPO_EINVAL, "part %d outside [0, %d)", part, np);
  if (np > 1 && (bufs->flags & MHPPO_ROLLOUT_VALU_POLICY))
    return set_error(MHPPO_EINVAL, "parts > 1: MFMA policy only");
  return rollout_policy(env, actor_cross, actor_wait, bufs, part, np, stream);
}

static int rollout_policy(mhppo_env *env, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                          mhppo_rollout_bufs *bufs, int part, int nparts, void *stream) {
  if (!env || !actor_cross || !actor_wait || !bufs) return set_error(MHPPO_EINVAL, "null argument");
  if (actor_cross->n_in != NF_C || actor_wait->n_in != NF_C || actor_cross->n_out != 1 || actor_wait->n_out != 1)
    return set_error(MHPPO_EINVAL, "continuous actors must be 13 -> 1");
  GUARD_DEVICE(env_device(env));
  const Cfg &c = env_cfg(env);
  size_t R = (size_t)c.N * c.nS * c.P;
  if (R > (size_t)INT32_MAX - 2) return set_error(MHPPO_EINVAL, "N*S*P too large");
  if (!bufs->rows) return set_error(MHPPO_EINVAL, "the policy step needs the head lists (bufs->rows)");
  if (!(bufs->flags & MHPPO_ROLLOUT_VALU_POLICY)) {
    // persistent 32-row MFMA tiles (grid below)
    const int dev = env_device(env);
    if (dev < 0 || dev >= mhppo::MAX_DEVICES) return set_error(MHPPO_EINVAL, "device %d >= %d", dev, mhppo::MAX_DEVICES);
    constexpr size_t WPB = PTPB / 64;  // waves per block
    const size_t tiles = R / (32 * (size_t)nparts) + 2;
    // at least the blocks that fit at once (this part's share of them), at most one tile per wave, and
    // beyond the resident blocks ~2 tiles per wave: the waiting blocks start as the first ones drain
    // (cfg4's 8 192 tiles per part: 1 024 blocks, collect -9 %; cfg3: 513, -2 %; cfg2: 65 at one tile
    // per wave, -7 %; profiles/r06_rollout/ab_policy_grid.txt)
    const size_t resident = (size_t)MHPPO_POLICY_BLOCKS_PER_CU * device_cus(dev) / nparts + 1;
    const size_t blocks = std::min<size_t>(std::max<size_t>(resident, (tiles + 2 * WPB - 1) / (2 * WPB)),
                                           (tiles + WPB - 1) / WPB);
    VLAUNCHB(k_policy_mfma, c.variant, dim3((unsigned)blocks), dim3(PTPB), 2 * pol::HEAD * sizeof(float),
             (hipStream_t)stream, c, actor_cross->packed, actor_wait->packed, actor_cross->mean, actor_cross->std,
             actor_wait->mean, actor_wait->std, *bufs, env_bufs(env), part, nparts);
    CHECK_HIP(hipGetLastError());
    return MHPPO_OK;
  }
#ifdef MHPPO_TEST_KERNELS
  // the VALU reference: one wave per 64 rows of one head (at most R/64 + 2 waves), or with
  // MHPPO_ROLLOUT_VALU_POLICY | MHPPO_ROLLOUT_VALU_UNSORTED the unsorted one-lane-per-row kernel
  if (bufs->flags & MHPPO_ROLLOUT_VALU_UNSORTED) {
    size_t shm = 2 * sizeof(float) * mlp_size(NF_C, 1);
    VLAUNCH(k_policy, c.variant, grid_for(R), shm, (hipStream_t)stream, c, *actor_cross, *actor_wait, *bufs);
  } else {
    const size_t waves = (R + 63) / 64 + 2;
    const dim3 grid((unsigned)((waves + TPB / 64 - 1) / (TPB / 64)));
    VLAUNCH(k_policy_sorted, c.variant, grid, 0, (hipStream_t)stream, c, actor_cross->packed, actor_wait->packed,
            actor_cross->mean, actor_cross->std, actor_wait->mean, actor_wait->std, *bufs, env_bufs(env));
  }
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
#else
  return set_error(MHPPO_EINVAL, "MHPPO_ROLLOUT_VALU_POLICY: the VALU policy kernels are in the test build only");
#endif
}

int mhppo_kernel_timing_begin(int n) {
  if (n < 0) return set_error(MHPPO_EINVAL, "kernel timing: n < 0");
  KernelTiming &k = g_ktime;
  k.on = false;
  k.used = 0;
  int dev = 0;
  CHECK_HIP(hipGetDevice(&dev));
  if (dev != k.dev) {  // events of another device: replace them
    for (hipEvent_t e : k.ev) (void)hipEventDestroy(e);
    k.ev.clear();
    k.cap = 0;
    k.dev = dev;
  }
  while ((int)k.ev.size() < 2 * n) {
    hipEvent_t e;
    CHECK_HIP(hipEventCreate(&e));
    k.ev.push_back(e);
  }
  if (n > k.cap) k.cap = n;
  k.on = n > 0;
  return MHPPO_OK;
}

static int kernel_timing_collect(double *ms_total, float *ms_each, int cap, int *launches) {
  KernelTiming &k = g_ktime;
  const int used = k.used;
  k.on = false;  // off before anything can fail: later launches are untimed either way
  k.used = 0;
  double tot = 0.0;
  for (int i = 0; i < used; i++) {
    CHECK_HIP(hipEventSynchronize(k.ev[2 * i + 1]));
    float ms = 0.f;
    CHECK_HIP(hipEventElapsedTime(&ms, k.ev[2 * i], k.ev[2 * i + 1]));
    tot += ms;
    if (ms_each && i < cap) ms_each[i] = ms;
  }
  if (ms_total) *ms_total = tot;
  if (launches) *launches = used;
  return MHPPO_OK;
}

int mhppo_kernel_timing_end(double *ms_total, int *launches) {
  return kernel_timing_collect(ms_total, nullptr, 0, launches);
}

int mhppo_kernel_timing_end_each(float *ms_each, int cap, int *launches) {
  if (cap < 0 || (cap > 0 && !ms_each)) return set_error(MHPPO_EINVAL, "kernel timing: bad output buffer");
  return kernel_timing_collect(nullptr, ms_each, cap, launches);
}

static int rollout_sample_env(mhppo_env *env, const float *eps, int t, mhppo_rollout_bufs *bufs, int part,
                              int nparts, void *stream) {
  if (!env || !eps || !bufs) return set_error(MHPPO_EINVAL, "null argument");
  if (t < 0 || t >= bufs->T) return set_error(MHPPO_EINVAL, "step %d outside [0, %d)", t, bufs->T);
  GUARD_DEVICE(env_device(env));
  const Cfg &c = env_cfg(env);
  // the compact layout with one pedestrian: the policy wrote each row's features at its record index,
  // which only the in-place record (feat_c = obs_c[t]) reads back at the right place
  if (bufs->rec_of && c.P == 1 && bufs->feat_c != bufs->obs_c + (size_t)t * c.N * c.nS * NF_C)
    return set_error(MHPPO_EINVAL, "rec_of with one pedestrian: feat_c must point at obs_c[t]");
  const int e_lo = part_env(c, part, nparts), e_hi = part_env(c, part + 1, nparts);
  if (e_hi <= e_lo) return MHPPO_OK;  // an empty part (N < 64 nparts)
#define SAMPLE_REG(V_, NC_, NAV_, NP_)                                                                      \
  if (launch_sample_reg<V_, NC_, NAV_, NP_>(c, env_bufs(env), eps, t, *bufs, (hipStream_t)stream, e_lo, e_hi)) { \
    CHECK_HIP(hipGetLastError());                                                                           \
    return MHPPO_OK;                                                                                        \
  }
  MHPPO_REG_SHAPES(SAMPLE_REG)
#undef SAMPLE_REG
  VLAUNCH(k_sample_env, c.variant, grid_for((size_t)(e_hi - e_lo)), 0, (hipStream_t)stream, c, env_bufs(env), eps, t,
          *bufs, e_lo, e_hi);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_rollout_sample_env(mhppo_env *env, const float *eps, int t, mhppo_rollout_bufs *bufs, void *stream) {
  return rollout_sample_env(env, eps, t, bufs, 0, 1, stream);
}

int mhppo_rollout_sample_env_part(mhppo_env *env, const float *eps, int t, mhppo_rollout_bufs *bufs, int part,
                                  void *stream) {
  if (!bufs) return set_error(MHPPO_EINVAL, "null argument");
  const int np = bufs->parts > 1 ? bufs->parts : 1;
  if (part < 0 || part >= np) return set_error(MHPPO_EINVAL, "part %d outside [0, %d)", part, np);
  return rollout_sample_env(env, eps, t, bufs, part, np, stream);
}

int mhppo_rollout_step(mhppo_env *env, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait, const float *eps,
                       int t, mhppo_rollout_bufs *bufs, void *stream) {
  int rc = mhppo_rollout_policy(env, actor_cross, actor_wait, bufs, stream);
  if (rc) return rc;
  return mhppo_rollout_sample_env(env, eps, t, bufs, stream);
}

int mhppo_rollout_check(mhppo_rollout_bufs *bufs, void *stream) {
  if (!bufs) return set_error(MHPPO_EINVAL, "null argument");
  if (!bufs->status) return MHPPO_OK;
  hipStream_t s = (hipStream_t)stream;
  uint32_t st = 0;
  CHECK_HIP(hipMemcpyAsync(&st, bufs->status, sizeof(st), hipMemcpyDeviceToHost, s));
  CHECK_HIP(hipStreamSynchronize(s));
  if (!st) return MHPPO_OK;
  CHECK_HIP(hipMemsetAsync(bufs->status, 0, sizeof(uint32_t), s));
  return set_error(MHPPO_ENAN, "NaN policy output sampled (%s%s%s): the reference raises ValueError here",
                   (st & 1u) ? "Categorical probs of the choice actor, :409" : "", (st & 3u) == 3u ? "; " : "",
                   (st & 2u) ? "MultivariateNormal loc of the continuous actors, :451" : "");
}

int mhppo_eval_step(mhppo_env *env, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                    const mhppo_mlp *actor_choice, int t, mhppo_eval_bufs *bufs, void *stream) {
  if (!env || !actor_cross || !actor_wait || !actor_choice || !bufs) return set_error(MHPPO_EINVAL, "null argument");
  // the histories (obs_hist, acts, rews_c, rews_d, waiting) may be NULL: their stores are skipped
  if (!bufs->obs || !bufs->a_d || !bufs->trig || !bufs->ep_min || !bufs->saved)
    return set_error(MHPPO_EINVAL, "eval bufs: obs, a_d, trig, ep_min and saved are required");
  const Cfg &c = env_cfg(env);
  if (actor_cross->n_in != NF_C || actor_wait->n_in != NF_C || actor_cross->n_out != 1 || actor_wait->n_out != 1)
    return set_error(MHPPO_EINVAL, "continuous actors must be 13 -> 1");
  if (actor_choice->n_in != choice_dim(c) || actor_choice->n_out != 2)
    return set_error(MHPPO_EINVAL, "choice actor must be %d -> 2", choice_dim(c));
  if (t < 0 || t >= bufs->T || t >= c.max_episode)
    return set_error(MHPPO_EINVAL, "step %d outside [0, %d)", t, bufs->T < c.max_episode ? bufs->T : c.max_episode);
  GUARD_DEVICE(env_device(env));
  size_t shm = sizeof(float) * (2 * mlp_size(NF_C, 1) + mlp_size(choice_dim(c), 2));
  VLAUNCH(k_eval_step, c.variant, grid_for(c.N), shm, (hipStream_t)stream, c, env_bufs(env), *actor_cross,
          *actor_wait, *actor_choice, t, *bufs);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}


}  // extern "C"
