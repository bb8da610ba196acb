// ppo_math.h — the scalar arithmetic the rollout, the losses and the train kernels share, free of
// the env (host+device): the MVN(loc, diag(0.5)) sample / log-prob constants, the clipped PPO
// surrogate with its gradient, torch.minimum, and Philox-4x32-10.  ppo_heads.h builds the heads'
// per-row arithmetic (finishes, Categorical, advantage, loss rows) on it.  rollout_dev.h includes
// it; the units that need nothing of the env include it alone (noise.hip, ppo_batch.hip) or through
// ppo_heads.h (ppo_loss.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef MHPPO_HD  // as env_dev.h defines it
#define MHPPO_HD __host__ __device__ __attribute__((always_inline))
#endif

namespace mhppo {

constexpr int NF_C = 13;  // obs_car_ped width (2 + 9 + 2)

// PPO clipped surrogate f = -min(r A, clamp(r, .8, 1.2) A) and df/dr, with torch's tie
// rule (minimum splits the gradient evenly on ties; clamp passes it on [0.8, 1.2]
// inclusive) — Coop-MH-PPO-scalable.py:803-806, :838-841
MHPPO_HD inline double surr_and_grad(double r, double A, double &dfdr) {
  double rc = r < 0.8 ? 0.8 : (r > 1.2 ? 1.2 : r);
  double s1 = r * A, s2 = rc * A;
  double in = (r >= 0.8 && r <= 1.2) ? 1.0 : 0.0;
  double g;
  if (s1 < s2)
    g = A;
  else if (s2 < s1)
    g = in * A;
  else
    g = 0.5 * A + 0.5 * in * A;
  dfdr = -g;
  return -(s1 < s2 ? s1 : s2);
}
// The same with the ratio's magnitude in float32 and its clip branch decided in float64 (the
// split-precision train kernel's continuous actor).  r = expf(lp - lp_old) carries ~2 float32
// roundings; which branch the reference's float64 ratio takes depends only on
// d = lp - lp_old in float64 (exact: a difference of two floats), against ln 0.8 / ln 1.2:
//   A > 0: -min(rA, clamp(r)A) follows r up to r = 1.2 (dfdr = -A), then is constant;
//   A < 0: it follows r from r = 0.8 on, and is constant below.
// (At r in [0.8, 1.2] the two terms tie and torch's minimum splits the gradient evenly between
// them, 0.5 A + 0.5 A.)  The thresholds are those of the correctly rounded float64 ratio exp(d):
// LN_0_8 is the smallest double whose exp rounds to >= 0.8 (the double), LN_1_2 the largest whose exp
// rounds to <= 1.2, two resp. three doubles beyond the rounded logarithms (-0x1.c8ff7c79a9a20p-3,
// 0x1.7565011e49675p-3): exp(d) is 0.8 resp. 1.2 exactly, a tie, for five resp. seven doubles around
// them (tests/test_rollout_math.py derives both in 60-digit arithmetic).  d is a multiple of 2^-24
// for log-densities below -0.5, whose grid points lie >= 8e-9 from ln 0.8 and ln 1.2: there the
// decision is the float64 ratio's whatever the exp
// (tests/test_update_scale_gpu.py counts the rows a float32 decision would flip).
constexpr double LN_0_8 = -0x1.c8ff7c79a9a22p-3, LN_1_2 = 0x1.7565011e49678p-3;
MHPPO_HD inline float surr_and_grad_fd(float r, double d, float A, float &dfdr) {
  const bool lo = d < LN_0_8, hi = d > LN_1_2;  // exp(d) < 0.8, > 1.2 in float64
  const float rc = lo ? 0.8f : (hi ? 1.2f : r);
  const bool follow = A > 0.0f ? !hi : (A < 0.0f && !lo);
  dfdr = follow ? -A : 0.0f;
  const float s1 = r * A, s2 = rc * A;
  return -(s1 < s2 ? s1 : s2);
}

// MVN(loc, diag(0.5)) in float32, the arithmetic torch performs (multivariate_normal.py
// rsample / log_prob; pinned bit for bit against torch in tests/test_rollout_math.py, as are the
// surrogates above and t_minimum below):
//   sample a = loc + L*eps;  x = (a - loc) * (1/L);  logp = -0.5*(log(2 pi) + x*x) - log(L)
constexpr float MVN_L = 0x1.6a09e6p-1f;        // cholesky([[0.5]]) in float32
constexpr float MVN_INV_L = 0x1.6a09e6p+0f;    // float32(1/L) as torch's triangular solve uses
constexpr float MVN_LOG2PI = 0x1.d67f1cp+0f;   // float32(1 * math.log(2*math.pi))
constexpr float MVN_HALF_LOGDET = -0x1.62e432p-2f;  // float32 log(L)

MHPPO_HD inline float mvn_sample(float loc, float eps) { return loc + MVN_L * eps; }
MHPPO_HD inline float mvn_logp(float a, float loc) {
  float x = (a - loc) * MVN_INV_L;
  float m = x * x;
  return (-0.5f * (MVN_LOG2PI + m)) - MVN_HALF_LOGDET;
}

// torch.minimum (NaN-propagating) in float32
MHPPO_HD inline float t_minimum(float a, float b) {
  if (a != a) return a;
  if (b != b) return b;
  return (b < a) ? b : a;
}

// Philox-4x32-10 (perf-mode noise)
MHPPO_HD inline void philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}
// The noise's draw `ctr` under `seed` (pinned against a reference written from the algorithm's
// definition in tests/test_noise_host.py and tests/test_noise_gpu.py): the Philox words of counter
// block (ctr lo, ctr hi, "mhpp", 0) under key (seed lo, seed hi); word 0's top 24 bits are the
// uniform in [0, 1); the normal is Box-Muller on u1 = (those + 1) 2^-24 in (0, 1] and word 1's u2.
MHPPO_HD inline void philox_words(uint64_t seed, uint64_t ctr, uint32_t w[4]) {
  w[0] = (uint32_t)ctr;
  w[1] = (uint32_t)(ctr >> 32);
  w[2] = 0x6d687070u;
  w[3] = 0u;
  philox(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}
MHPPO_HD inline float philox_u24(uint32_t w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }
MHPPO_HD inline float philox_box_muller(uint32_t w0, uint32_t w1) {
  const float u1 = ((float)(w0 >> 8) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
  const float u2 = philox_u24(w1);
  return sqrtf(-2.0f * logf(u1)) * cosf(6.2831853071795865f * u2);
}
// the one draw function of the noise kernels and the host harness (tools/hostfwd.cpp)
MHPPO_HD inline float philox_draw(uint64_t seed, uint64_t ctr, bool normal) {
  uint32_t w[4];
  philox_words(seed, ctr, w);
  if (normal) return philox_box_muller(w[0], w[1]);
  return philox_u24(w[0]);
}

}  // namespace mhppo
