// policy_sample_rule.h — the training (stochastic) policy as a function of an observation row
// (host+device): what the collector does between reading `o` and its env step (k_choice in
// rollout.hip, k_policy_mfma in rollout_policy.h, sample_env_body in rollout_step.h), restated once
// on the featurizers of rollout_dev.h, the heads of ppo_heads.h and the MVN / Philox arithmetic of
// ppo_math.h.
//   sample_decide (row r, slot i, ped p): obs_car_ped_d -> choice net -> softmax_pair -> cat_normalise
//           -> a_d = u >= n[0] (or the forced value), logp_d = logf(cat_clamp(n[a_d]));
//           per (row, slot): closest = closest_ped_d, exist = the car's exist field (scalable) or 1
//   sample_act (row r, slot i): loc = 2.0f, sel = 0; for p ascending over the candidates that take
//           part (ped_gate): out = the output of the head a_d[i][p] picks, loc = t_minimum(loc, out),
//           sel = p where out == loc; a = mvn_sample(loc, eps), logp = mvn_logp(a, loc);
//           actions[i] = a, actions[S + i] = 2 a_d[i][closest[i]] - 1 (the collector's light, not the
//           evaluation's flat-index light_of); the recorded feature row is obs_car_ped(o, i, sel)
// No override and no cap.  NaN probabilities set status bit 1, a NaN loc status bit 2 (k_choice,
// sample_env_body).
// An absent car slot of the scalable variant (exist 0) has no record in the collector, but the
// collector computes its action like any other slot's and hands it to the env step, where it reaches
// present slots' rewards; so does this rule: the slot is computed as any other, and its
// sample, log-probability and feature row are the caller's to mask with `exist`.
// The noise is a tape (u [M, S, P] or forced [M, S, P] for decide, eps [M, S] for act) or drawn here
// by philox_draw at the collector's counters (RolloutGPU.draw_noise): row r is env first_env + r,
//   uniform (r, i, p): counter (first_env + r) S P + i P + p
//   normal  (r, i) at step t: counter (t + 1) 2^40 + (first_env + r) S + i
// under key = seed * 1000003 + iteration (mod 2^64).  Both are linear in the launch's flat index.
// The pieces are what the MFMA kernels of policy_infer.hip run per triple; sample_decide_row /
// sample_act_row chain them over one row with the VALU mlp_forward and are what tools/hostpolicy.cpp
// loops over rows.  The collector's kernels keep their own statement of the rule;
// tests/test_policy_sample_gpu.py pins the two against each other bit for bit.
#pragma once
#include "policy_rule.h"

namespace mhppo {
namespace policy {

// One launch's noise: tape (or, for decide, forced) when set, else Philox under (key, first_env, t)
struct SampleNoise {
  const float *tape;
  const int32_t *forced;
  uint64_t key, first_env;
  int64_t t;
};
// q: the launch's flat triple index (r S + i) P + p
MHPPO_HD inline float noise_uniform(const SampleNoise &z, int64_t q, int SP) {
  return z.tape ? z.tape[q] : philox_draw(z.key, z.first_env * (uint64_t)SP + (uint64_t)q, false);
}
// u: the launch's flat (row, slot) index r S + i
MHPPO_HD inline float noise_normal(const SampleNoise &z, int64_t u, int S) {
  return z.tape ? z.tape[u]
                : philox_draw(z.key, ((uint64_t)(z.t + 1) << 40) + z.first_env * (uint64_t)S + (uint64_t)u, true);
}

// Categorical(probs) of the choice net's pair: the draw (u >= n[0], or `forced` when has_forced) and
// its log-probability; p0, p1 the softmax (NaN: status bit 1, probs_nan)
MHPPO_HD inline int sample_choice(float z0, float z1, float u, bool has_forced, int forced, float &p0, float &p1,
                                  float &logp) {
  softmax_pair<LibmRollout>(z0, z1, p0, p1);
  float n[2];
  cat_normalise(p0, p1, n);
  const int a = has_forced ? forced : (u >= n[0] ? 1 : 0);
  logp = logf(cat_clamp(a ? n[1] : n[0]));
  return a;
}
MHPPO_HD inline bool probs_nan(float p0, float p1) { return p0 != p0 || p1 != p1; }
// the slot's car is there (the scalable variant's exist field; every other variant: always)
MHPPO_HD inline uint8_t slot_exist(const float *o, const ObsLayout &L, int i) {
  return L.scalable ? (uint8_t)(o[i * L.cw + 6] != 0.0f) : (uint8_t)1;
}
// pedestrian p is a candidate of a slot's fold: the scalable `if exist:` gate on the pedestrian
MHPPO_HD inline bool ped_gate(const float *o, const ObsLayout &L, int p) {
  return !L.scalable || o[L.ped_off + 9 * p + 7] != 0.0f;
}
// one candidate folded into the slot's loc (torch.minimum; the last pedestrian equal to the running min is kept)
MHPPO_HD inline void fold_sample(float &loc, int &sel, float out, int p) {
  loc = t_minimum(loc, out);
  if (out == loc) sel = p;
}
// the collector's light: the decision of the slot's closest pedestrian (ad_row: the row's [S, P]
// block; a `closest` outside [0, P) reads pedestrian 0)
MHPPO_HD inline double sample_light(const int32_t *ad_row, int P, int i, int closest) {
  const int cl = (unsigned)closest < (unsigned)P ? closest : 0;
  return (double)(2 * ad_row[i * P + cl] - 1);
}

// One observation row r of a launch, every (slot, ped).  Outputs: a_d / logp_d [S, P], probs
// [S, P, 2] or NULL, feat_d [S, P, dc] or NULL, closest / exist [S]; returns the row's status bits.
MHPPO_HD inline uint32_t sample_decide_row(const float *o, const ObsLayout &L, const float *Wd, int dc,
                                           const SampleNoise &nz, int64_t r, int32_t *a_d, float *logp_d, float *probs,
                                           float *feat_d, int32_t *closest, uint8_t *exist) {
  uint32_t st = 0;
  const int SP = L.S * L.P;
  for (int i = 0; i < L.S; i++) {
    closest[i] = closest_ped_d(o, L, i);
    exist[i] = slot_exist(o, L, i);
    for (int p = 0; p < L.P; p++) {
      const int k = i * L.P + p;
      const int64_t q = r * SP + k;
      float fd[2 + 6 * (MAXS - 1) + 10], z[2], p0, p1;
      obs_car_ped_d(o, L, i, p, fd);
      if (feat_d)
        for (int c = 0; c < dc; c++) feat_d[k * dc + c] = fd[c];
      mlp_forward<0, 2>(Wd, dc, fd, z);
      const float u = nz.forced ? 0.0f : noise_uniform(nz, q, SP);
      a_d[k] = sample_choice(z[0], z[1], u, nz.forced != nullptr, nz.forced ? nz.forced[q] : 0, p0, p1, logp_d[k]);
      if (probs_nan(p0, p1)) st |= 1u;
      if (probs) {
        probs[2 * k] = p0;
        probs[2 * k + 1] = p1;
      }
    }
  }
  return st;
}

// One observation row r with its decisions a_d [S, P] and closest [S]: actions [2 S], act / logp [S],
// feat_c [S, 13] or NULL; returns the row's status bits.
MHPPO_HD inline uint32_t sample_act_row(const float *o, const ObsLayout &L, const ContNet &cross, const ContNet &wait,
                                        const int32_t *a_d, const int32_t *closest, const SampleNoise &nz, int64_t r,
                                        double *actions, float *act, float *logp, float *feat_c) {
  uint32_t st = 0;
  for (int i = 0; i < L.S; i++) {
    float loc = 2.0f;  // torch.tensor(car_b[1, 0])
    int sel = 0;
    for (int p = 0; p < L.P; p++) {
      if (!ped_gate(o, L, p)) continue;
      float f[NF_C], z;
      obs_car_ped(o, L, i, p, f);
      const ContNet &m = uses_wait(a_d[i * L.P + p]) ? wait : cross;
      mlp_forward<NF_C, 1>(m.W, NF_C, f, &z);
      fold_sample(loc, sel, finish_cont<LibmRollout>(z, m.mean, m.std), p);
    }
    if (loc != loc) st |= 2u;
    const float a = mvn_sample(loc, noise_normal(nz, r * L.S + i, L.S));
    act[i] = a;
    logp[i] = mvn_logp(a, loc);
    actions[i] = (double)a;
    actions[L.S + i] = sample_light(a_d, L.P, i, closest[i]);
    if (feat_c) obs_car_ped(o, L, i, sel, feat_c + i * NF_C);
  }
  return st;
}

}  // namespace policy
}  // namespace mhppo
