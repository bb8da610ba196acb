// hostpolicy.cpp — the stateless policy (mhppo_policy_dims / _decide / _act) on the CPU, from the
// device source: csrc/policy_rule.h's decide_row / act_row looped over observation rows, on the
// featurizers and the VALU mlp_forward of csrc/rollout_dev.h and the heads of csrc/ppo_heads.h.  The CPU
// reference of tests/test_policy_host.py and tests/test_policy_gpu.py.
// Built with -ffp-contract=off: the fmaf chains are exact.
// Build: make -C tools   ->  tools/libhostpolicy.so (ctypes, tools/hostpolicy.py)
#include <stdint.h>

#include "../mh-ppo_amd/csrc/policy_rule.h"

using namespace mhppo;
using namespace mhppo::policy;

extern "C" {
// out = (obs_dim, S, P, choice_dim); -1: the config is refused
int hp_dims(const mhppo_env_cfg *cfg, int32_t *out) {
  Cfg c;
  if (cfg_from(cfg, c)) return -1;
  dims_of(c, out);
  return 0;
}

// obs [M, obs_dim] -> a_d int32 [M, S, P], probs [M, S, P, 2] or NULL.  Wd: torch-packed, choice_dim inputs
int hp_decide(const mhppo_env_cfg *cfg, const float *Wd, const float *obs, int64_t M, int32_t *a_d, float *probs) {
  Cfg c;
  if (cfg_from(cfg, c)) return -1;
  const ObsLayout L = obs_layout(c);
  const int dc = choice_dim(c), SP = c.nS * c.P;
  for (int64_t r = 0; r < M; r++)
    decide_row(obs + r * L.obs_dim, L, Wd, dc, a_d + r * SP, probs ? probs + 2 * r * SP : nullptr);
  return 0;
}

// obs [M, obs_dim], a_d int32 [M, S, P] -> actions float64 [M, 2 S]
int hp_act(const mhppo_env_cfg *cfg, const float *Wc, float mean_c, float std_c, const float *Ww, float mean_w,
           float std_w, const float *obs, const int32_t *a_d, int64_t M, double *actions) {
  Cfg c;
  if (cfg_from(cfg, c)) return -1;
  const ObsLayout L = obs_layout(c);
  const ContNet cross{Wc, mean_c, std_c}, wait{Ww, mean_w, std_w};
  for (int64_t r = 0; r < M; r++)
    act_row(obs + r * L.obs_dim, L, c.dt, c.b00, c.b10, cross, wait, a_d + r * c.nS * c.P, actions + r * 2 * c.nS);
  return 0;
}

// the 13 obs_car_ped features of every (row, slot, ped): [M, S, P, 13] (which rows are left-lane or capped)
int hp_features(const mhppo_env_cfg *cfg, const float *obs, int64_t M, float *feat) {
  Cfg c;
  if (cfg_from(cfg, c)) return -1;
  const ObsLayout L = obs_layout(c);
  for (int64_t r = 0; r < M; r++)
    for (int i = 0; i < c.nS; i++)
      for (int p = 0; p < c.P; p++) obs_car_ped(obs + r * L.obs_dim, L, i, p, feat + ((r * c.nS + i) * c.P + p) * NF_C);
  return 0;
}

// the obs_car_ped_d choice features of every (row, slot, ped): [M, S, P, choice_dim]
int hp_features_d(const mhppo_env_cfg *cfg, const float *obs, int64_t M, float *feat) {
  Cfg c;
  if (cfg_from(cfg, c)) return -1;
  const ObsLayout L = obs_layout(c);
  const int dc = choice_dim(c);
  for (int64_t r = 0; r < M; r++)
    for (int i = 0; i < c.nS; i++)
      for (int p = 0; p < c.P; p++) obs_car_ped_d(obs + r * L.obs_dim, L, i, p, feat + ((r * c.nS + i) * c.P + p) * dc);
  return 0;
}
}
