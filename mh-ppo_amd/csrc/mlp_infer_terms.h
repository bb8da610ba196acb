// mlp_infer_terms.h — what follows a Model_PPO head's last layer outside the rollout, and the
// per-row terms of the PPO diagnostics (host+device: mlp_infer.hip runs them on the GPU,
// tools/hostfwd.cpp compiles this very source for the CPU reference).
//
// The head finishes restate the rollout's, operation for operation: finish_cont is
// k_policy_mfma's tanh * std + mean (two roundings, Model_PPO :87-89), finish_choice k_choice's
// pairwise softmax (:81-85), choice_logp its Categorical log-prob (normalise, clamp to
// [eps, 1 - eps], logf; torch/distributions/utils.py).  With the same weights and feature row they
// return the rollout's bits, so a diagnostic d = logp_new - logp_old is exactly 0 before an update.
#pragma once
#include "../../include/mhppo.h"
#include "libm_glibc.h"
#include "rollout_dev.h"

namespace mhppo {
namespace infer {

constexpr int N_IN_MAX = 64;  // widest input (the scalable 8-slot choice head: 54)

MHPPO_HD inline float finish_cont(float z, float mean, float std) {
  float t = mhppo_tanhf(z) * std;
  return t + mean;
}

MHPPO_HD inline void finish_choice(float z0, float z1, float &p0, float &p1) {
  float mx = z0 > z1 ? z0 : z1;
  float ex0 = mhppo_expf(z0 - mx), ex1 = mhppo_expf(z1 - mx);
  float s = ex0 + ex1;
  p0 = ex0 / s;
  p1 = ex1 / s;
}

// Categorical(probs).log_prob(a) as k_choice writes it; n0 / n1: the normalised, clamped pair
MHPPO_HD inline float choice_logp(float p0, float p1, int a, float &n0, float &n1) {
  const float eps = 1.1920928955078125e-07f, hi = 1.0f - 1.1920928955078125e-07f;
  float sum = p0 + p1;
  n0 = p0 / sum;
  n1 = p1 / sum;
  n0 = n0 < eps ? eps : (n0 > hi ? hi : n0);
  n1 = n1 < eps ? eps : (n1 > hi ? hi : n1);
  return logf(a ? n1 : n0);
}

// entropy of that pair in float64
MHPPO_HD inline double choice_entropy(float n0, float n1) {
  const double a = (double)n0, b = (double)n1;
  return -(a * log(a) + b * log(b));
}

// The actor's terms of one row (t: double [MHPPO_DIAG_N], entries DSUM .. ENT written).
// d = logp_new - logp_old is exact in float64 (a difference of two floats); the clip decision is
// the train kernels' (ppo_math.h surr_and_grad_fd: d against float64 ln 0.8 / ln 1.2).
MHPPO_HD inline double actor_terms(float logp_new, float logp_old, double ent, double *t) {
  const double d = (double)logp_new - (double)logp_old;
  t[MHPPO_DIAG_DSUM] = d;
  t[MHPPO_DIAG_K3] = expm1(d) - d;
  t[MHPPO_DIAG_CLIP] = (d < LN_0_8 || d > LN_1_2) ? 1.0 : 0.0;
  t[MHPPO_DIAG_RATIO] = exp(d);
  t[MHPPO_DIAG_ENT] = ent;
  return d;
}

// The critic's terms of one row (entries E .. V written)
MHPPO_HD inline void critic_terms(float ret, float V, double *t) {
  const double g = (double)ret, v = (double)V, e = g - v;
  t[MHPPO_DIAG_E] = e;
  t[MHPPO_DIAG_E2] = e * e;
  t[MHPPO_DIAG_G] = g;
  t[MHPPO_DIAG_G2] = g * g;
  t[MHPPO_DIAG_V] = v;
}

// One row of the diagnostics from the nets' raw outputs: za[] the actor's pre-finish outputs
// (1 for kind 1, 2 for kind 2), vc the critic's output.  act: the row's action (kind 1: the float
// action; kind 2: 0 / 1).  Returns d; *lp_new (optional) = logp_new.
MHPPO_HD inline double diag_row(int kind, const float *za, float mean, float std, float vc, float act_f, int act_i,
                                float logp_old, float ret, double *t, float *lp_new) {
  float lp;
  double ent = 0.0;
  if (kind == 2) {
    float p0, p1, n0, n1;
    finish_choice(za[0], za[1], p0, p1);
    lp = choice_logp(p0, p1, act_i, n0, n1);
    ent = choice_entropy(n0, n1);
  } else {
    lp = mvn_logp(act_f, finish_cont(za[0], mean, std));
  }
  if (lp_new) *lp_new = lp;
  critic_terms(ret, vc, t);
  return actor_terms(lp, logp_old, ent, t);
}

}  // namespace infer
}  // namespace mhppo
