// mlp_infer.hip — forward-only kernels of a Model_PPO head outside the rollout (+ C-ABI):
//   k_mlp_forward  one net over [M, n_in] rows, per-row output (Model_PPO.forward_rows);
//   k_ppo_diag     actor and critic of one head over its batch, float64 sums of the per-row PPO
//                  diagnostics (approximate KL, clip fraction, entropy, explained variance);
//   k_ppo_kl       the actor alone over the same batch: the two KL sums of the diagnostics, bit for
//                  bit, cheap enough for every epoch (the KL early stop's measurement).
// All run 32-row tiles on f32 MFMA in the rollout's arithmetic (mlp_infer_tile.h): a wave stages
// its tile's rows through LDS with coalesced loads, the nets' permuted weight images are staged
// once per block, and a block walks its tiles in a fixed order (grid-stride), so the sums depend
// only on M.  The per-row terms are the host+device functions of mlp_infer_terms.h; the block
// partials of the diagnostics are folded by block_prims.h's k_fold.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/mhppo.h"
#include "block_prims.h"
#include "common.h"
#include "mlp_infer_terms.h"
#include "mlp_infer_tile.h"

using namespace mhppo;
using namespace mhppo::infer;

namespace {
constexpr int ITPB = 256, IWAVES = ITPB / 64;
// blocks of a launch: one 32-row tile per wave and step, at most MAX_BLOCKS blocks (two resident
// per CU on 256 CUs: k_ppo_diag's register bound) walking the rest grid-stride.  A function of M alone: the order
// of the diagnostics' sums, and with it their bits, is the same on every device.
constexpr int MAX_BLOCKS = 512;
int n_blocks(int64_t M) { return (int)std::min<int64_t>((n_tiles(M) + IWAVES - 1) / IWAVES, MAX_BLOCKS); }

struct NetArg {
  const float *W;
  float mean, std;
};

// LDS: [image][IWAVES input tiles]
template <int NOUT>
__global__ void __launch_bounds__(ITPB) k_mlp_forward(NetArg net, int kind, int n_in, const float *__restrict__ X,
                                                      int64_t M, float *__restrict__ out) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, l = tid & 63, j = l & 31, kh = l >> 5, w = tid >> 6;
  const Img g = img_layout(n_in, NOUT);
  float *xs = lds + g.size + w * xtile_floats(g);
  stage_image<ITPB>(lds, g, net.W, n_in, NOUT, tid);
  zero_x_pad(xs, g, n_in, l);
  const XStage xst = xstage_init(n_in, l);
  const int64_t ntiles = (M + 31) / 32, stride = (int64_t)gridDim.x * IWAVES;
  // every wave of the block runs the same number of steps (the barriers below)
  for (int64_t t0 = (int64_t)blockIdx.x * IWAVES; t0 < ntiles; t0 += stride) {
    const int64_t tile = t0 + w;
    const bool live = tile < ntiles;
    const int64_t r0 = tile * 32;
    const int nr = !live ? 0 : (M - r0 < 32 ? (int)(M - r0) : 32);
    if (live) stage_x(xs, g, xst, X, r0, nr, n_in, l);
    __syncthreads();  // the staged tile (and, at the first step, the image) is visible
    if (live) {
      float z[NOUT];
      tile_forward<NOUT>(lds, g, xs, j, kh, z);
      if (kh == 0 && j < nr) {
        const int64_t r = r0 + j;
        if (NOUT == 2) {
          float p0, p1;
          softmax_pair<LibmRollout>(z[0], z[NOUT - 1], p0, p1);
          out[2 * r] = p0;
          out[2 * r + 1] = p1;
        } else {
          out[r] = kind == 1 ? finish_cont<LibmRollout>(z[0], net.mean, net.std) : z[0];
        }
      }
    }
    __syncthreads();  // all reads of the tile done before the next step overwrites it
  }
}

// LDS: [actor image][critic image][IWAVES input tiles][MHPPO_DIAG_N x IWAVES doubles]
// partials: [MHPPO_DIAG_N][gridDim.x]
// Registers for two waves per SIMD (213 VGPRs at kind 1, 249 at kind 2, no scratch): without the
// bound the accumulators go to AGPRs on top of as many VGPRs and the kernel runs one wave per SIMD;
// bound for three (<= 168) it spills.  One wave's MFMA chain covers the other's float64 epilogue.
template <int KIND>
__global__ void __launch_bounds__(ITPB) __attribute__((amdgpu_waves_per_eu(2)))
    k_ppo_diag(NetArg actor, NetArg critic, int n_in, const float *__restrict__ X, int64_t M, const void *act,
               const float *__restrict__ logp_old, const float *__restrict__ ret, double *__restrict__ partials) {
  constexpr int NA = KIND == 2 ? 2 : 1;
  extern __shared__ float lds[];
  const int tid = threadIdx.x, l = tid & 63, j = l & 31, kh = l >> 5, w = tid >> 6;
  const Img ga = img_layout(n_in, NA), gc = img_layout(n_in, 1);
  float *La = lds, *Lc = La + ga.size;
  float *xs = Lc + gc.size + w * xtile_floats(ga);
  double *wsum = reinterpret_cast<double *>(Lc + gc.size + IWAVES * xtile_floats(ga));
  stage_image<ITPB>(La, ga, actor.W, n_in, NA, tid);
  stage_image<ITPB>(Lc, gc, critic.W, n_in, 1, tid);
  zero_x_pad(xs, ga, n_in, l);
  const XStage xst = xstage_init(n_in, l);
  double acc[MHPPO_DIAG_N];
#pragma unroll
  for (int k = 0; k < MHPPO_DIAG_N; k++) acc[k] = 0.0;
  const int64_t ntiles = (M + 31) / 32, stride = (int64_t)gridDim.x * IWAVES;
  for (int64_t t0 = (int64_t)blockIdx.x * IWAVES; t0 < ntiles; t0 += stride) {
    const int64_t tile = t0 + w;
    const bool live = tile < ntiles;
    const int64_t r0 = tile * 32;
    const int nr = !live ? 0 : (M - r0 < 32 ? (int)(M - r0) : 32);
    if (live) stage_x(xs, ga, xst, X, r0, nr, n_in, l);
    __syncthreads();
    if (live) {
      const bool mine = kh == 0 && j < nr;
      const int64_t r = r0 + j;
      // the row's scalars, issued ahead of the forwards
      float act_f = 0.0f, lp_old = 0.0f, g_ret = 0.0f;
      int act_i = 0;
      if (mine) {
        if (KIND == 2) act_i = static_cast<const int32_t *>(act)[r];
        else act_f = static_cast<const float *>(act)[r];
        lp_old = logp_old[r];
        g_ret = ret[r];
      }
      float za[NA], zc[1];
      // one net at a time (interleaved, both forwards' accumulators would be live at once)
      tile_forward<NA>(La, ga, xs, j, kh, za);
      __builtin_amdgcn_sched_barrier(0);
      tile_forward<1>(Lc, gc, xs, j, kh, zc);
      __builtin_amdgcn_sched_barrier(0);
      if (mine) {
        double t[MHPPO_DIAG_N];
        diag_row(KIND, za, actor.mean, actor.std, zc[0], act_f, act_i, lp_old, g_ret, t, nullptr);
#pragma unroll
        for (int k = 0; k < MHPPO_DIAG_N; k++) acc[k] += t[k];
      }
    }
    __syncthreads();
  }
  // block partial in a fixed order: a shuffle tree per wave, then the waves in index order
#pragma unroll
  for (int k = 0; k < MHPPO_DIAG_N; k++) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (l == 0) wsum[k * IWAVES + w] = v;
  }
  __syncthreads();
  if (tid < MHPPO_DIAG_N) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < IWAVES; q++) s += wsum[tid * IWAVES + q];
    partials[(size_t)tid * gridDim.x + blockIdx.x] = s;
  }
}

// The actor half of k_ppo_diag alone, for the KL early stop's per-epoch measurement: one weight
// image, one tile_forward, the two float64 sums DSUM and K3; `ret` is not read.  The grid
// (n_blocks(M)), the tile-to-wave walk, the rows' terms (actor_row), the per-wave shuffle tree, the
// wave order and the fold are k_ppo_diag's, so the two sums carry the diagnostics' bits.
// LDS: [actor image][IWAVES input tiles][MHPPO_KL_N x IWAVES doubles]
// partials: [MHPPO_KL_N][gridDim.x]
// Registers (gfx950): 106 VGPRs at kind 1, 119 at kind 2, no AGPRs, no scratch, no VGPR spill (kind 2
// parks 2 SGPRs in VGPR lanes), both under the 128 of four waves per SIMD, which is the bound asked
// for: left free, the compiler puts the accumulators in AGPRs and lands at three waves; bound for
// five it goes to scratch.  What bounds the occupancy per head width is in DESIGN.md ("KL early
// stopping": the grid's cap of 512 blocks comes first).
constexpr int MHPPO_KL_N = 2;
template <int KIND>
__global__ void __launch_bounds__(ITPB) __attribute__((amdgpu_waves_per_eu(4)))
    k_ppo_kl(NetArg actor, int n_in, const float *__restrict__ X, int64_t M, const void *act,
             const float *__restrict__ logp_old, double *__restrict__ partials) {
  constexpr int NA = KIND == 2 ? 2 : 1;
  static_assert(MHPPO_DIAG_DSUM == 0 && MHPPO_DIAG_K3 == 1, "the KL launch keeps the first two diagnostics terms");
  extern __shared__ float lds[];
  const int tid = threadIdx.x, l = tid & 63, j = l & 31, kh = l >> 5, w = tid >> 6;
  const Img ga = img_layout(n_in, NA);
  float *La = lds;
  float *xs = La + ga.size + w * xtile_floats(ga);
  double *wsum = reinterpret_cast<double *>(La + ga.size + IWAVES * xtile_floats(ga));
  stage_image<ITPB>(La, ga, actor.W, n_in, NA, tid);
  zero_x_pad(xs, ga, n_in, l);
  const XStage xst = xstage_init(n_in, l);
  double acc[MHPPO_KL_N] = {0.0, 0.0};
  const int64_t ntiles = (M + 31) / 32, stride = (int64_t)gridDim.x * IWAVES;
  for (int64_t t0 = (int64_t)blockIdx.x * IWAVES; t0 < ntiles; t0 += stride) {
    const int64_t tile = t0 + w;
    const bool live = tile < ntiles;
    const int64_t r0 = tile * 32;
    const int nr = !live ? 0 : (M - r0 < 32 ? (int)(M - r0) : 32);
    if (live) stage_x(xs, ga, xst, X, r0, nr, n_in, l);
    __syncthreads();
    if (live) {
      const bool mine = kh == 0 && j < nr;
      const int64_t r = r0 + j;
      // the row's scalars, issued ahead of the forward
      float act_f = 0.0f, lp_old = 0.0f;
      int act_i = 0;
      if (mine) {
        if (KIND == 2) act_i = static_cast<const int32_t *>(act)[r];
        else act_f = static_cast<const float *>(act)[r];
        lp_old = logp_old[r];
      }
      float za[NA];
      tile_forward<NA>(La, ga, xs, j, kh, za);
      if (mine) {
        double t[MHPPO_DIAG_ENT + 1];
        actor_row(KIND, za, actor.mean, actor.std, act_f, act_i, lp_old, t, nullptr);
#pragma unroll
        for (int k = 0; k < MHPPO_KL_N; k++) acc[k] += t[k];
      }
    }
    __syncthreads();
  }
  // block partial in k_ppo_diag's order: a shuffle tree per wave, then the waves in index order
#pragma unroll
  for (int k = 0; k < MHPPO_KL_N; k++) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (l == 0) wsum[k * IWAVES + w] = v;
  }
  __syncthreads();
  if (tid < MHPPO_KL_N) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < IWAVES; q++) s += wsum[tid * IWAVES + q];
    partials[(size_t)tid * gridDim.x + blockIdx.x] = s;
  }
}

// sums[k] = the fold of term k's block partials (one chain per thread, then the tree), written
constexpr auto k_diag_fold = k_fold<ITPB, 1, false>;

int check_net(const mhppo_mlp *m, const char *what) {
  if (!m || !m->packed) return set_error(MHPPO_EINVAL, "%s: null pointer", what);
  if (m->n_in < 1 || m->n_in > N_IN_MAX)
    return set_error(MHPPO_EINVAL, "%s: n_in %d outside 1..%d", what, (int)m->n_in, N_IN_MAX);
  if (m->kind < 0 || m->kind > 2) return set_error(MHPPO_EINVAL, "%s: kind %d is not 0, 1 or 2", what, (int)m->kind);
  const int want = m->kind == 2 ? 2 : 1;
  if (m->n_out != want)
    return set_error(MHPPO_EINVAL, "%s: kind %d needs n_out %d, not %d", what, (int)m->kind, want, (int)m->n_out);
  return MHPPO_OK;
}

// dynamic LDS above the 64 KB a kernel gets by default (the wide choice heads' diagnostics); the
// kernel is the template argument, so each instantiation has a limit table of its own
template <auto KERNEL>
int allow_lds(size_t bytes) {
  static LdsLimit limit;
  return allow_dynamic_lds(reinterpret_cast<const void *>(KERNEL), bytes, limit);
}
}  // namespace

extern "C" {

int mhppo_mlp_forward(const mhppo_mlp *net, const float *X, int64_t M, float *out, void *stream) {
  if (int rc = check_net(net, "mhppo_mlp_forward")) return rc;
  if (M < 0) return set_error(MHPPO_EINVAL, "mhppo_mlp_forward: M < 0");
  if (M == 0) return MHPPO_OK;
  if (!X || !out) return set_error(MHPPO_EINVAL, "mhppo_mlp_forward: null pointer");
  const NetArg a{net->packed, net->mean, net->std};
  const Img g = img_layout(net->n_in, net->n_out);
  const size_t shm = ((size_t)g.size + (size_t)IWAVES * xtile_floats(g)) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)n_blocks(M));
  if (net->n_out == 2) {
    if (int rc = allow_lds<k_mlp_forward<2>>(shm)) return rc;
    hipLaunchKernelGGL(k_mlp_forward<2>, grid, dim3(ITPB), shm, s, a, (int)net->kind, (int)net->n_in, X, M, out);
  } else {
    if (int rc = allow_lds<k_mlp_forward<1>>(shm)) return rc;
    hipLaunchKernelGGL(k_mlp_forward<1>, grid, dim3(ITPB), shm, s, a, (int)net->kind, (int)net->n_in, X, M, out);
  }
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int64_t mhppo_ppo_diag_work_bytes(int64_t M) {
  if (M <= 0) return 8;
  return (int64_t)MHPPO_DIAG_N * n_blocks(M) * (int64_t)sizeof(double);
}

int mhppo_ppo_diag(const mhppo_mlp *actor, const mhppo_mlp *critic, const float *X, int64_t M, const void *act,
                   const float *logp_old, const float *ret, double *sums, void *work, void *stream) {
  if (int rc = check_net(actor, "mhppo_ppo_diag actor")) return rc;
  if (int rc = check_net(critic, "mhppo_ppo_diag critic")) return rc;
  if (actor->kind == 0) return set_error(MHPPO_EINVAL, "mhppo_ppo_diag: the actor is kind 0 (a critic)");
  if (critic->kind != 0) return set_error(MHPPO_EINVAL, "mhppo_ppo_diag: the critic is kind %d, not 0", (int)critic->kind);
  if (actor->n_in != critic->n_in)
    return set_error(MHPPO_EINVAL, "mhppo_ppo_diag: actor n_in %d != critic n_in %d", (int)actor->n_in,
                     (int)critic->n_in);
  if (M < 0) return set_error(MHPPO_EINVAL, "mhppo_ppo_diag: M < 0");
  if (!sums) return set_error(MHPPO_EINVAL, "mhppo_ppo_diag: null pointer (sums)");
  hipStream_t s = (hipStream_t)stream;
  if (M == 0) {
    CHECK_HIP(hipMemsetAsync(sums, 0, MHPPO_DIAG_N * sizeof(double), s));
    return MHPPO_OK;
  }
  if (!X || !act || !logp_old || !ret || !work) return set_error(MHPPO_EINVAL, "mhppo_ppo_diag: null pointer");
  const NetArg a{actor->packed, actor->mean, actor->std}, c{critic->packed, 0.0f, 1.0f};
  const Img ga = img_layout(actor->n_in, actor->n_out), gc = img_layout(critic->n_in, 1);
  const size_t shm = ((size_t)ga.size + gc.size + (size_t)IWAVES * xtile_floats(ga)) * sizeof(float) +
                     (size_t)MHPPO_DIAG_N * IWAVES * sizeof(double);
  const int nb = n_blocks(M);
  double *part = static_cast<double *>(work);
  if (actor->kind == 2) {
    if (int rc = allow_lds<k_ppo_diag<2>>(shm)) return rc;
    hipLaunchKernelGGL(k_ppo_diag<2>, dim3(nb), dim3(ITPB), shm, s, a, c, (int)actor->n_in, X, M, act, logp_old, ret,
                       part);
  } else {
    if (int rc = allow_lds<k_ppo_diag<1>>(shm)) return rc;
    hipLaunchKernelGGL(k_ppo_diag<1>, dim3(nb), dim3(ITPB), shm, s, a, c, (int)actor->n_in, X, M, act, logp_old, ret,
                       part);
  }
  hipLaunchKernelGGL(k_diag_fold, dim3(MHPPO_DIAG_N), dim3(ITPB), 0, s, part, nb, sums);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int64_t mhppo_ppo_kl_work_bytes(int64_t M) {
  if (M <= 0) return 8;
  return (int64_t)MHPPO_KL_N * n_blocks(M) * (int64_t)sizeof(double);
}

int mhppo_ppo_kl(const mhppo_mlp *actor, const float *X, int64_t M, const void *act, const float *logp_old,
                 double *sums, void *work, void *stream) {
  if (int rc = check_net(actor, "mhppo_ppo_kl actor")) return rc;
  if (actor->kind == 0) return set_error(MHPPO_EINVAL, "mhppo_ppo_kl: the actor is kind 0 (a critic)");
  if (M < 0) return set_error(MHPPO_EINVAL, "mhppo_ppo_kl: M < 0");
  if (!sums) return set_error(MHPPO_EINVAL, "mhppo_ppo_kl: null pointer (sums)");
  hipStream_t s = (hipStream_t)stream;
  if (M == 0) {
    CHECK_HIP(hipMemsetAsync(sums, 0, MHPPO_KL_N * sizeof(double), s));
    return MHPPO_OK;
  }
  if (!X || !act || !logp_old || !work) return set_error(MHPPO_EINVAL, "mhppo_ppo_kl: null pointer");
  const NetArg a{actor->packed, actor->mean, actor->std};
  const Img ga = img_layout(actor->n_in, actor->n_out);
  const size_t shm = ((size_t)ga.size + (size_t)IWAVES * xtile_floats(ga)) * sizeof(float) +
                     (size_t)MHPPO_KL_N * IWAVES * sizeof(double);
  const int nb = n_blocks(M);
  double *part = static_cast<double *>(work);
  if (actor->kind == 2) {
    if (int rc = allow_lds<k_ppo_kl<2>>(shm)) return rc;
    hipLaunchKernelGGL(k_ppo_kl<2>, dim3(nb), dim3(ITPB), shm, s, a, (int)actor->n_in, X, M, act, logp_old, part);
  } else {
    if (int rc = allow_lds<k_ppo_kl<1>>(shm)) return rc;
    hipLaunchKernelGGL(k_ppo_kl<1>, dim3(nb), dim3(ITPB), shm, s, a, (int)actor->n_in, X, M, act, logp_old, part);
  }
  hipLaunchKernelGGL(k_diag_fold, dim3(MHPPO_KL_N), dim3(ITPB), 0, s, part, nb, sums);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

}  // extern "C"
