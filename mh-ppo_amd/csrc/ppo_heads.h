// ppo_heads.h — the per-row arithmetic of the PPO heads, one copy for every kernel (host+device):
// what turns a head's last-layer output into a policy (finish_cont, softmax_pair, cat_normalise,
// cat_clamp), the advantage's normalisation (adv_moments, adv_normalised) and the loss rows of the
// update (cont_logp_x, cont_dmu, choice_term, cat_grad_p, softmax_jacobian).  With ppo_math.h's
// surr_and_grad / mvn_logp it is all a kernel needs between the last layer and dL/dy;
// tools/hostfwd.cpp compiles this very source for the CPU tests (tests/test_ppo_heads_host.py).
//
// Two libm flavours, kept apart on purpose (the Libm template parameter of the functions that call
// tanhf / expf):
//   LibmRollout  the glibc restatements of libm_glibc.h.  The rollout side (k_choice, the policy
//                kernels, k_eval_step, mlp_infer): its actions and probabilities are compared bit
//                for bit with the C oracle, which runs the host's glibc.
//   LibmUpdate   the platform's own tanhf / expf (the device's in a kernel, the host's in
//                tools/hostfwd.cpp).  The update side (mlp_x3.h, mlp_train_f32.h, ppo_loss.hip): it
//                is judged against float64 autograd within a float32 error bound, and the device's
//                functions are the cheaper ones.
// logf and the float64 exp / sqrt are the platform's on both sides.
// Everything is built with -ffp-contract=off: an a * b + c written here is two roundings.
#pragma once
#include <math.h>

#include "libm_glibc.h"
#include "ppo_math.h"

namespace mhppo {

struct LibmRollout {
  static MHPPO_HD inline float tanh(float x) { return mhppo_tanhf(x); }
  static MHPPO_HD inline float exp(float x) { return mhppo_expf(x); }
};
struct LibmUpdate {
  static MHPPO_HD inline float tanh(float x) { return tanhf(x); }
  static MHPPO_HD inline float exp(float x) { return expf(x); }
};

// ---------------------------------------------------------------- forward
// Model_PPO type 1 (:87-89): tanh(z) * std + mean, two roundings; t = tanh(z) (its backward's 1 - t*t)
template <class Libm>
MHPPO_HD inline float finish_cont(float z, float mean, float std, float &t) {
  t = Libm::tanh(z);
  return t * std + mean;
}
template <class Libm>
MHPPO_HD inline float finish_cont(float z, float mean, float std) {
  float t;
  return finish_cont<Libm>(z, mean, std, t);
}

// Model_PPO type 2 (:81-85): softmax over the pair, shifted by the max as torch does.
// The max is fmaxf; the rollout used to write z0 > z1 ? z0 : z1.  The two give the same p0, p1:
//   ordered, unequal logits      the same max;
//   equal logits, +0 and -0      whichever the max, z - mx is +-0 for both and exp(+-0) = 1;
//   one NaN logit                the ternary takes z1 (NaN or not), fmaxf the other logit: either way
//                                the NaN logit's own exp is NaN, so s is NaN and both p are NaN;
//   two equal infinities         inf - inf = NaN in both forms: both p are NaN (so is +inf with a
//                                finite logit; -inf with a finite one gives (0, 1) in both forms).
// A NaN's sign and payload are not pinned; k_choice's status flag tests p != p.
template <class Libm>
MHPPO_HD inline void softmax_pair(float z0, float z1, float &p0, float &p1) {
  const float mx = fmaxf(z0, z1);
  const float e0 = Libm::exp(z0 - mx), e1 = Libm::exp(z1 - mx);
  const float se = e0 + e1;
  p0 = e0 / se;
  p1 = e1 / se;
}

// Categorical(probs) (torch/distributions/utils.py): pn = p / (p0 + p1), returns the sum;
// clamp_probs: pn into [eps, 1 - eps], eps = float32's machine epsilon
constexpr float CAT_EPS = 1.1920928955078125e-07f, CAT_HI = 1.0f - CAT_EPS;
MHPPO_HD inline float cat_normalise(float p0, float p1, float (&pn)[2]) {
  const float sp = p0 + p1;
  pn[0] = p0 / sp;
  pn[1] = p1 / sp;
  return sp;
}
MHPPO_HD inline float cat_clamp(float pn_k) { return pn_k < CAT_EPS ? CAT_EPS : (pn_k > CAT_HI ? CAT_HI : pn_k); }

// The advantage's mean and torch.std (unbiased) from the critic pass's float64 sums
// stats = (sum A, sum A^2) over the m_global rows (:786-787), rounded once to float32
MHPPO_HD inline void adv_moments(const double *stats, double m_global, float &meanf, float &stdf) {
  double mean = stats[0] / m_global;
  double var = (stats[1] - stats[0] * mean) / (m_global - 1.0);
  meanf = (float)mean;
  stdf = (float)sqrt(var > 0 ? var : 0.0);
}
// (A - mean) / (std + 1e-10) in float32 (:787)
MHPPO_HD inline float adv_normalised(float a, float meanf, float stdf) { return (a - meanf) / (stdf + 1e-10f); }

// ---------------------------------------------------------------- loss rows
// MVN(mu, 0.5).log_prob(action) at update time (:800): the action is float64 there, so the
// difference is taken in float64 and rounded, then torch's float32 solve and tail; x = diff / L.
// (The rounded exact difference of two floats is their float32 difference, so this returns
// mvn_logp's bits: tests/test_ppo_heads_host.py.  mvn_logp stays the rollout's form.)
MHPPO_HD inline float cont_logp_x(float act, float mu, float &x) {
  const float diff = (float)((double)act - (double)mu);
  x = diff * MVN_INV_L;
  return (-0.5f * (MVN_LOG2PI + x * x)) - MVN_HALF_LOGDET;
}
// dL/dmu of the row: dlogp/dmu = x / L (d/dmu of -0.5 ((a - mu) / L)^2), times dL/dr * r / M
MHPPO_HD inline float cont_dmu(double inv_m, double dfdr, double r, float x) {
  return (float)(inv_m * dfdr * r * (double)x * (double)MVN_INV_L);
}
MHPPO_HD inline float cont_dmu(double inv_m, float dfdr, float r, float x) {
  return (float)(inv_m * (double)dfdr * (double)r * (double)x * (double)MVN_INV_L);
}

// One action k of the choice actor's surrogate (:834-842 in its O(M) form): the clamped
// probability's log, the float64 ratio against `old`, fk = the surrogate; returns dL/dpn_k for the
// weight w_k (clamp_probs passes the gradient on [eps, 1 - eps] inclusive, as torch.clamp does).
// The caller accumulates w_k * fk.
MHPPO_HD inline double choice_term(float pn_k, double old, double A, double w_k, double inv_m2, double &fk) {
  const float pc = cat_clamp(pn_k);
  const double r = exp((double)logf(pc) - old);
  double dfdr;
  fk = surr_and_grad(r, A, dfdr);
  const double pass = (pn_k >= CAT_EPS && pn_k <= CAT_HI) ? 1.0 : 0.0;
  return inv_m2 * w_k * dfdr * r * pass / (double)pc;
}
// dL/dp_k through pn_k = p_k / (p0 + p1); sp = p0 + p1
MHPPO_HD inline void cat_grad_p(const double (&dlp)[2], const float (&pn)[2], float sp, double &g0, double &g1) {
  const double sd = (double)sp;
  g0 = (dlp[0] * (1.0 - pn[0]) - dlp[1] * pn[1]) / sd;
  g1 = (dlp[1] * (1.0 - pn[1]) - dlp[0] * pn[0]) / sd;
}
// dL/dy through p = softmax(y): p_k (g_k - sum_j p_j g_j)
MHPPO_HD inline void softmax_jacobian(const float (&p)[2], double g0, double g1, float &dy0, float &dy1) {
  const double dot = (double)p[0] * g0 + (double)p[1] * g1;
  dy0 = (float)((double)p[0] * (g0 - dot));
  dy1 = (float)((double)p[1] * (g1 - dot));
}

}  // namespace mhppo
