// ppo_loss.hip — the update-time losses on flat batches (+ C-ABI): advantage statistics and
// normalisation (mhppo_adv_stats / _adv_normalize), the clipped PPO surrogates of the continuous
// and the choice actors (mhppo_ppo_cont_fwd_bwd / _ppo_choice_fwd_bwd) and the critic's MSE
// (mhppo_mse_fwd_bwd), each with its gradient.  Elementwise kernels plus deterministic two-pass
// reductions in float64 (a fixed summation order, block_prims.h: the same call gives the same
// bits); the block partials live in the per-device scratch (common.h), in stream order.
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/mhppo.h"
#include "block_prims.h"
#include "common.h"
#include "launch1d.h"
#include "ppo_math.h"  // surr_and_grad, the MVN constants

using namespace mhppo;

namespace {

// ------------------------------------------------- deterministic reductions
// Pass 1 writes one partial per block (block_prims.h block_sum: the fixed tree); pass 2 folds the
// partials into out[k] (+=) with k_fold_add.  NP = partial arrays per call.
template <int NP>
__device__ inline void block_reduce_store(double (&v)[NP], double *partials, int nblocks) {
  block_sum<TPB>(v);
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < NP; k++) partials[(size_t)k * nblocks + blockIdx.x] = v[k];
}
constexpr auto k_fold_add = k_fold<TPB, 1, true>;

__global__ void __launch_bounds__(TPB) k_adv_stats(const float *ret, const float *val, int64_t M, double *partials) {
  int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  double v[2] = {0.0, 0.0};
  if (i < M) {
    float a = ret[i] - val[i];  // rtgs_batch - V_batch (float32, :786)
    v[0] = a;
    v[1] = (double)a * (double)a;
  }
  block_reduce_store<2>(v, partials, gridDim.x);
}

// (A - mean) / (std + 1e-10), torch.std unbiased (:787)
__global__ void __launch_bounds__(TPB)
    k_adv_norm(const float *ret, const float *val, int64_t M, const double *stats, double mg, float *adv) {
  int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= M) return;
  double mean = stats[0] / mg;
  double var = (stats[1] - stats[0] * mean) / (mg - 1.0);
  float meanf = (float)mean, stdf = (float)sqrt(var > 0 ? var : 0.0);
  float a = ret[i] - val[i];
  adv[i] = (a - meanf) / (stdf + 1e-10f);
}

__global__ void __launch_bounds__(TPB)
    k_ppo_cont(const float *mu, const float *act, const float *lp_old, const float *adv, int64_t M, double inv_m,
               float *dmu, double *partials) {
  int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  double v[1] = {0.0};
  if (i < M) {
    // log_prob(action f64) (:800): diff in float64 then float32 solve, float32 tail
    float diff = (float)((double)act[i] - (double)mu[i]);
    float x = diff * MVN_INV_L;
    float lp = (-0.5f * (MVN_LOG2PI + x * x)) - MVN_HALF_LOGDET;
    double r = exp((double)lp - (double)lp_old[i]);  // float64 ratio (:803)
    double dfdr;
    double f = surr_and_grad(r, (double)adv[i], dfdr);
    v[0] = f;
    // dlogp/dmu = x / L  (d/dmu of -0.5 ((a - mu)/L)^2)
    dmu[i] = (float)(inv_m * dfdr * r * (double)x * (double)MVN_INV_L);
  }
  block_reduce_store<1>(v, partials, gridDim.x);
}

// O(M) form of the M x M Categorical broadcast (:834-842)
__global__ void __launch_bounds__(TPB)
    k_ppo_choice(const float *probs, const float *lp_old, const float *adv, int64_t M, const double *counts,
                 double inv_m2, float *dprobs, double *partials) {
  int64_t j = (int64_t)blockIdx.x * TPB + threadIdx.x;
  double v[1] = {0.0};
  if (j < M) {
    const float eps = 1.1920928955078125e-07f, hi = 1.0f - 1.1920928955078125e-07f;
    float p0 = probs[2 * j], p1 = probs[2 * j + 1];
    float s = p0 + p1;
    float pn[2] = {p0 / s, p1 / s};
    double A = adv[j], old = lp_old[j];
    double dlp[2];
    double f = 0.0;
    for (int k = 0; k < 2; k++) {
      float pc = pn[k] < eps ? eps : (pn[k] > hi ? hi : pn[k]);
      float lp = logf(pc);
      double r = exp((double)lp - old);
      double dfdr;
      double fk = surr_and_grad(r, A, dfdr);
      f += counts[k] * fk;
      double pass = (pn[k] >= eps && pn[k] <= hi) ? 1.0 : 0.0;
      dlp[k] = inv_m2 * counts[k] * dfdr * r * pass / (double)pc;  // dL/dpn_k
    }
    v[0] = f;
    // pn_k = p_k / (p0 + p1)
    double sd = (double)s;
    double g0 = (dlp[0] * (1.0 - pn[0]) - dlp[1] * pn[1]) / sd;
    double g1 = (dlp[1] * (1.0 - pn[1]) - dlp[0] * pn[0]) / sd;
    dprobs[2 * j] = (float)g0;
    dprobs[2 * j + 1] = (float)g1;
  }
  block_reduce_store<1>(v, partials, gridDim.x);
}

__global__ void __launch_bounds__(TPB)
    k_mse(const float *val, const float *ret, int64_t M, double inv_m, float *dv, double *partials) {
  int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  double v[1] = {0.0};
  if (i < M) {
    float d = val[i] - ret[i];
    v[0] = (double)d * (double)d;
    dv[i] = (float)(2.0 * inv_m * (double)d);
  }
  block_reduce_store<1>(v, partials, gridDim.x);
}

}  // namespace

extern "C" {

int mhppo_adv_stats(const float *ret, const float *value, int64_t M, double *stats, void *stream) {
  if (M == 0) return MHPPO_OK;  // an empty shard (data parallel) adds nothing; its pointers may be NULL
  if (!ret || !value || !stats || M < 0) return set_error(MHPPO_EINVAL, "bad argument");
  dim3 g = grid_for(M);
  double *part = scratch(2 * (size_t)g.x);
  if (!part) return set_error(MHPPO_ENOMEM, "scratch allocation failed");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_adv_stats, g, dim3(TPB), 0, s, ret, value, M, part);
  hipLaunchKernelGGL(k_fold_add, dim3(2), dim3(TPB), 0, s, part, (int)g.x, stats);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_adv_normalize(const float *ret, const float *value, int64_t M, const double *stats, double m_global,
                        float *adv, void *stream) {
  if (M == 0) return MHPPO_OK;
  if (!ret || !value || !stats || !adv || M < 0) return set_error(MHPPO_EINVAL, "bad argument");
  hipLaunchKernelGGL(k_adv_norm, grid_for(M), dim3(TPB), 0, (hipStream_t)stream, ret, value, M, stats, m_global,
                     adv);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_ppo_cont_fwd_bwd(const float *mu, const float *act, const float *logp_old, const float *adv, int64_t M,
                           double inv_m, float *dmu, double *loss, void *stream) {
  if (M == 0) return MHPPO_OK;
  if (!mu || !act || !logp_old || !adv || !dmu || !loss || M < 0) return set_error(MHPPO_EINVAL, "bad argument");
  dim3 g = grid_for(M);
  double *part = scratch(g.x);
  if (!part) return set_error(MHPPO_ENOMEM, "scratch allocation failed");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ppo_cont, g, dim3(TPB), 0, s, mu, act, logp_old, adv, M, inv_m, dmu, part);
  hipLaunchKernelGGL(k_fold_add, dim3(1), dim3(TPB), 0, s, part, (int)g.x, loss);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_ppo_choice_fwd_bwd(const float *probs, const float *logp_old, const float *adv, int64_t M,
                             const double *counts, double inv_m2, float *dprobs, double *loss, void *stream) {
  if (M == 0) return MHPPO_OK;
  if (!probs || !logp_old || !adv || !counts || !dprobs || !loss || M < 0)
    return set_error(MHPPO_EINVAL, "bad argument");
  dim3 g = grid_for(M);
  double *part = scratch(g.x);
  if (!part) return set_error(MHPPO_ENOMEM, "scratch allocation failed");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_ppo_choice, g, dim3(TPB), 0, s, probs, logp_old, adv, M, counts, inv_m2, dprobs, part);
  hipLaunchKernelGGL(k_fold_add, dim3(1), dim3(TPB), 0, s, part, (int)g.x, loss);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_mse_fwd_bwd(const float *value, const float *ret, int64_t M, double inv_m, float *dv, double *loss,
                      void *stream) {
  if (M == 0) return MHPPO_OK;
  if (!value || !ret || !dv || !loss || M < 0) return set_error(MHPPO_EINVAL, "bad argument");
  dim3 g = grid_for(M);
  double *part = scratch(g.x);
  if (!part) return set_error(MHPPO_ENOMEM, "scratch allocation failed");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_mse, g, dim3(TPB), 0, s, value, ret, M, inv_m, dv, part);
  hipLaunchKernelGGL(k_fold_add, dim3(1), dim3(TPB), 0, s, part, (int)g.x, loss);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

}  // extern "C"
