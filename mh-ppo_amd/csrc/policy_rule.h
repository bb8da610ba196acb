// policy_rule.h — the deterministic policy as a function of an observation row (host+device): what
// k_eval_step (rollout_step.h) does between reading `o` and calling env_step_one, restated once on
// the featurizers of rollout_dev.h and the heads of ppo_heads.h.
//   decide  (row, slot i, ped p): obs_car_ped_d -> choice net -> softmax_pair -> a_d = p1 > p0
//   act     (row, slot i): a = b10; for p ascending: the triple's candidate (the left-lane override
//           or the mean action of the head a_d picks), a = min(a, cand) keeping the first on ties,
//           then the (10 - V) / dt cap
//   lights  actions[S + i] = 2 a_d[i] - 1 with the FLAT index i into the row's [S, P] block (the
//           reference's quirk, kept)
// Comparisons with NaN are false: a NaN head output changes nothing and is reported nowhere.
// The pieces (choice_of, override_cand, head_cand, fold_cand, light_of) are what the MFMA kernels
// of policy_infer.hip run per triple; decide_row / act_row chain them over one row with the VALU
// mlp_forward and are what tools/hostpolicy.cpp loops over rows (the CPU reference of the tests).
// k_eval_step keeps its own statement of the rule; tests/test_policy_gpu.py pins the two against
// each other bit for bit.
#pragma once
#include "env_body.h"  // build_cfg, MAXS
#include "ppo_heads.h"
#include "rollout_dev.h"

namespace mhppo {
namespace policy {

constexpr int MAX_P = 32;  // a (row, slot) group's pedestrians share one 32-row tile

// torch.argmax over the pair: the first maximum
MHPPO_HD inline int choice_of(float z0, float z1, float &p0, float &p1) {
  softmax_pair<LibmRollout>(z0, z1, p0, p1);
  return (p1 > p0) ? 1 : 0;
}
// the head a choice selects: wait when action_d = 2 a_d - 1 is positive
MHPPO_HD inline bool uses_wait(int a_d) { return (2 * a_d - 1) > 0; }
// the (10 - V) / dt cap, float64 from the float32 speed feature
MHPPO_HD inline double speed_cap(float v, double dt) { return (10.0 - (double)v) / dt; }
// the pedestrian left the lane (f[7] != 0): speed-limit tracking, clamped to the car's bounds
MHPPO_HD inline double override_cand(float v, double dt, double b00, double b10) {
  const double x = speed_cap(v, dt);
  const double m = (b10 < x) ? b10 : x;
  return (b00 > m) ? b00 : m;
}
// the head's mean action from its last-layer output
MHPPO_HD inline double head_cand(float z, float mean, float std) { return (double)finish_cont<LibmRollout>(z, mean, std); }
// one pedestrian folded into the slot's action (Python min keeps the first on ties), then the cap
MHPPO_HD inline void fold_cand(double &a, double cand, double lim) {
  if (cand < a) a = cand;
  if (lim < a) a = lim;
}
// ad_row: the row's a_d block [S, P]
MHPPO_HD inline double light_of(const int32_t *ad_row, int i) { return (double)(2 * ad_row[i] - 1); }

// One observation row, every (slot, ped): a_d [S, P]; probs [S, P, 2] or NULL.  Wd: the choice
// actor, torch-packed, dc inputs.
MHPPO_HD inline void decide_row(const float *o, const ObsLayout &L, const float *Wd, int dc, int32_t *a_d,
                                float *probs) {
  for (int i = 0; i < L.S; i++)
    for (int p = 0; p < L.P; p++) {
      float fd[2 + 6 * (MAXS - 1) + 10], z[2], p0, p1;
      obs_car_ped_d(o, L, i, p, fd);
      mlp_forward<0, 2>(Wd, dc, fd, z);
      a_d[i * L.P + p] = choice_of(z[0], z[1], p0, p1);
      if (probs) {
        probs[2 * (i * L.P + p)] = p0;
        probs[2 * (i * L.P + p) + 1] = p1;
      }
    }
}

struct ContNet {
  const float *W;  // torch-packed 13 -> 1
  float mean, std;
};
// One observation row with its decisions a_d [S, P]: actions [2 S] = [acc.., light..]
MHPPO_HD inline void act_row(const float *o, const ObsLayout &L, double dt, double b00, double b10,
                             const ContNet &cross, const ContNet &wait, const int32_t *a_d, double *actions) {
  for (int i = 0; i < L.S; i++) {
    double a = b10;
    for (int p = 0; p < L.P; p++) {
      float f[NF_C];
      obs_car_ped(o, L, i, p, f);
      double cand;
      if (f[7] != 0.0f) {
        cand = override_cand(f[0], dt, b00, b10);
      } else {
        const ContNet &m = uses_wait(a_d[i * L.P + p]) ? wait : cross;
        float z;
        mlp_forward<NF_C, 1>(m.W, NF_C, f, &z);
        cand = head_cand(z, m.mean, m.std);
      }
      fold_cand(a, cand, speed_cap(f[0], dt));
    }
    actions[i] = a;
  }
  for (int i = 0; i < L.S; i++) actions[L.S + i] = light_of(a_d, i);
}

// host: the variant and shape checks of mhppo_env_create, then build_cfg (n_envs, the seeds and
// flags play no part).  NULL, or why the config is refused.
inline const char *cfg_from(const mhppo_env_cfg *cfg, Cfg &c) {
  if (!cfg) return "null config";
  if (cfg->variant < 0 || cfg->variant > 5) return "unknown variant";
  if (cfg->nb_car < 1 || cfg->nb_ped < 1 || cfg->nb_lines < 1) return "bad nb_car/nb_ped/nb_lines";
  const int64_t nS = cfg->variant == V_SCALABLE ? 2 * (int64_t)cfg->nb_lines
                                                : (cfg->variant == V_4CARS2 ? 2 : 1) * (int64_t)cfg->nb_car;
  if (nS > MAXS) return "too many car slots";
  if (cfg->nb_ped > (1 << 20)) return "too many pedestrians";
  build_cfg(*cfg, c);
  return nullptr;
}
// obs_dim, S, P, choice_dim
inline void dims_of(const Cfg &c, int32_t out[4]) {
  out[0] = c.obs_dim;
  out[1] = c.nS;
  out[2] = c.P;
  out[3] = choice_dim(c);
}

}  // namespace policy
}  // namespace mhppo
