// mlp_infer_terms.h — the per-row terms of the PPO diagnostics (host+device: mlp_infer.hip runs
// them on the GPU, tools/hostfwd.cpp compiles this very source for the CPU reference).
//
// The head finishes are the rollout's own functions (ppo_heads.h, the LibmRollout flavour):
// finish_cont is the policy kernels' tanh * std + mean, softmax_pair k_choice's pairwise softmax,
// cat_normalise / cat_clamp its Categorical log-prob.  With the same weights and feature row they
// return the rollout's bits, so a diagnostic d = logp_new - logp_old is exactly 0 before an update.
#pragma once
#include "../../include/mhppo.h"
#include "ppo_heads.h"
#include "rollout_dev.h"

namespace mhppo {
namespace infer {

constexpr int N_IN_MAX = 64;  // widest input (the scalable 8-slot choice head: 54)

// entropy of the normalised, clamped pair in float64
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

// The actor half of one row from the actor's raw outputs: the head's finish, logp_new, then
// actor_terms (t entries DSUM .. ENT written).  za[] the pre-finish outputs (1 for kind 1, 2 for
// kind 2), act the row's action (kind 1: the float action; kind 2: 0 / 1).  Returns d; *lp_new
// (optional) = logp_new.  The one copy both k_ppo_diag and k_ppo_kl run: the KL launch's two sums
// are the diagnostics' DSUM and K3 terms, row for row (a caller that reads only those leaves the
// clip, ratio and entropy terms to the compiler's dead-code elimination).
MHPPO_HD inline double actor_row(int kind, const float *za, float mean, float std, float act_f, int act_i,
                                 float logp_old, double *t, float *lp_new) {
  float lp;
  double ent = 0.0;
  if (kind == 2) {
    float p0, p1, n[2];
    softmax_pair<LibmRollout>(za[0], za[1], p0, p1);
    cat_normalise(p0, p1, n);
    n[0] = cat_clamp(n[0]);
    n[1] = cat_clamp(n[1]);
    lp = logf(act_i ? n[1] : n[0]);  // Categorical(probs).log_prob(a) as k_choice writes it
    ent = choice_entropy(n[0], n[1]);
  } else {
    lp = mvn_logp(act_f, finish_cont<LibmRollout>(za[0], mean, std));
  }
  if (lp_new) *lp_new = lp;
  return actor_terms(lp, logp_old, ent, t);
}

// One row of the diagnostics from the nets' raw outputs: actor_row's arguments, vc the critic's
// output.  Returns d; *lp_new (optional) = logp_new.
MHPPO_HD inline double diag_row(int kind, const float *za, float mean, float std, float vc, float act_f, int act_i,
                                float logp_old, float ret, double *t, float *lp_new) {
  critic_terms(ret, vc, t);
  return actor_row(kind, za, mean, std, act_f, act_i, logp_old, t, lp_new);
}

}  // namespace infer
}  // namespace mhppo
