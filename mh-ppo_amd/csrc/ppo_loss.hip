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
#include "ppo_heads.h"  // the heads' per-row arithmetic; surr_and_grad (ppo_math.h)

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
  float meanf, stdf;
  adv_moments(stats, mg, meanf, stdf);
  adv[i] = adv_normalised(ret[i] - val[i], meanf, stdf);
}

__global__ void __launch_bounds__(TPB)
    k_ppo_cont(const float *mu, const float *act, const float *lp_old, const float *adv, int64_t M, double inv_m,
               float *dmu, double *partials) {
  int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  double v[1] = {0.0};
  if (i < M) {
    float x;
    float lp = cont_logp_x(act[i], mu[i], x);  // log_prob(action f64) (:800)
    double r = exp((double)lp - (double)lp_old[i]);  // float64 ratio (:803)
    double dfdr;
    double f = surr_and_grad(r, (double)adv[i], dfdr);
    v[0] = f;
    dmu[i] = cont_dmu(inv_m, dfdr, r, x);
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
    float pn[2];
    const float s = cat_normalise(probs[2 * j], probs[2 * j + 1], pn);
    double A = adv[j], old = lp_old[j];
    double dlp[2];
    double f = 0.0;
    for (int k = 0; k < 2; k++) {
      double fk;
      dlp[k] = choice_term(pn[k], old, A, counts[k], inv_m2, fk);
      f += counts[k] * fk;  // every term, as the count-weighted sum is written (the train kernels skip weight 0)
    }
    v[0] = f;
    double g0, g1;
    cat_grad_p(dlp, pn, s, g0, g1);
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
