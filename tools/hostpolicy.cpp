// hostpolicy.cpp — the stateless policy (mhppo_policy_dims / _decide / _act) on the CPU, from the
// device source: csrc/policy_rule.h's decide_row / act_row looped over observation rows, on the
// featurizers and the VALU mlp_forward of csrc/rollout_dev.h and the heads of csrc/ppo_heads.h.  The CPU
// reference of tests/test_policy_host.py and tests/test_policy_gpu.py.  hp_sample_decide / hp_sample_act
// do the same for the stochastic rule (csrc/policy_sample_rule.h: sample_decide_row / sample_act_row;
// tests/test_policy_sample_host.py, tests/test_policy_sample_gpu.py), hp_sample_noise is its noise alone.
// Built with -ffp-contract=off: the fmaf chains are exact.
// The row loops of the four rules run on hp_set_threads' threads (rows are independent and each writes
// its own outputs; a thread takes one contiguous run of rows), so a reference over 10^5 rows costs a
// fraction of a second (tests/test_tile_walk_gpu.py); one thread is the plain loop
// (tests/test_policy_sample_host.py: the same bits).
// Build: make -C tools   ->  tools/libhostpolicy.so (ctypes, tools/hostpolicy.py)
#include <stdint.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../mh-ppo_amd/csrc/policy_rule.h"
#include "../mh-ppo_amd/csrc/policy_sample_rule.h"

using namespace mhppo;
using namespace mhppo::policy;

namespace {
constexpr int MAX_THREADS = 16;
int g_threads = 0;  // 0: the machine's, MAX_THREADS at most

// body(lo, hi) -> status bits of rows [lo, hi), run on one thread per contiguous run of [0, M); the OR of the results
template <class Body>
uint32_t for_rows(int64_t M, Body body) {
  const int hw = (int)std::thread::hardware_concurrency();
  const int want = g_threads > 0 ? g_threads : std::min(MAX_THREADS, std::max(1, hw));
  const int nt = (int)std::min<int64_t>(want, std::max<int64_t>(M, 1));
  if (nt <= 1) return body(0, M);
  std::vector<uint32_t> st(nt, 0u);
  std::vector<std::thread> pool;
  const int64_t per = (M + nt - 1) / nt;
  for (int k = 0; k < nt; k++)
    pool.emplace_back([&, k] { st[k] = body(std::min(M, k * per), std::min(M, (k + 1) * per)); });
  uint32_t all = 0;
  for (int k = 0; k < nt; k++) {
    pool[k].join();
    all |= st[k];
  }
  return all;
}
}  // namespace

extern "C" {
// the row loops' thread count from here on: 1 .. 16, 0: the machine's (16 at most).  Returns the previous setting
int hp_set_threads(int n) {
  const int old = g_threads;
  g_threads = n < 0 ? 0 : std::min(n, MAX_THREADS);
  return old;
}

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
  for_rows(M, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; r++)
      decide_row(obs + r * L.obs_dim, L, Wd, dc, a_d + r * SP, probs ? probs + 2 * r * SP : nullptr);
    return 0u;
  });
  return 0;
}

// obs [M, obs_dim], a_d int32 [M, S, P] -> actions float64 [M, 2 S]
int hp_act(const mhppo_env_cfg *cfg, const float *Wc, float mean_c, float std_c, const float *Ww, float mean_w,
           float std_w, const float *obs, const int32_t *a_d, int64_t M, double *actions) {
  Cfg c;
  if (cfg_from(cfg, c)) return -1;
  const ObsLayout L = obs_layout(c);
  const ContNet cross{Wc, mean_c, std_c}, wait{Ww, mean_w, std_w};
  for_rows(M, [&](int64_t lo, int64_t hi) {
    for (int64_t r = lo; r < hi; r++)
      act_row(obs + r * L.obs_dim, L, c.dt, c.b00, c.b10, cross, wait, a_d + r * c.nS * c.P, actions + r * 2 * c.nS);
    return 0u;
  });
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

// The stochastic rule.  Noise: u (decide) / eps (act) the tape, forced the decisions themselves, all
// NULL: Philox under (key, first_env, t) at the collector's counters.
// obs [M, obs_dim] -> a_d int32, logp_d [M, S, P]; probs [M, S, P, 2] or NULL; feat_d [M, S, P, choice_dim]
// or NULL; closest int32, exist uint8 [M, S]; status uint32 [1] or NULL (OR-ed into)
int hp_sample_decide(const mhppo_env_cfg *cfg, const float *Wd, const float *obs, int64_t M, const float *u,
                     const int32_t *forced, uint64_t key, uint64_t first_env, int32_t *a_d, float *logp_d, float *probs,
                     float *feat_d, int32_t *closest, uint8_t *exist, uint32_t *status) {
  Cfg c;
  if (cfg_from(cfg, c)) return -1;
  if (u && forced) return -1;
  const ObsLayout L = obs_layout(c);
  const int dc = choice_dim(c), SP = c.nS * c.P;
  const SampleNoise nz{u, forced, key, first_env, 0};
  const uint32_t st = for_rows(M, [&](int64_t lo, int64_t hi) {
    uint32_t s = 0;
    for (int64_t r = lo; r < hi; r++)
      s |= sample_decide_row(obs + r * L.obs_dim, L, Wd, dc, nz, r, a_d + r * SP, logp_d + r * SP,
                             probs ? probs + 2 * r * SP : nullptr, feat_d ? feat_d + r * SP * dc : nullptr,
                             closest + r * c.nS, exist + r * c.nS);
    return s;
  });
  if (status) *status |= st;
  return 0;
}

// obs [M, obs_dim], a_d int32 [M, S, P], closest int32 [M, S] -> actions float64 [M, 2 S], act / logp
// float32 [M, S], feat_c [M, S, 13] or NULL
int hp_sample_act(const mhppo_env_cfg *cfg, const float *Wc, float mean_c, float std_c, const float *Ww, float mean_w,
                  float std_w, const float *obs, const int32_t *a_d, const int32_t *closest, int64_t M,
                  const float *eps, uint64_t key, uint64_t first_env, int64_t t, double *actions, float *act,
                  float *logp, float *feat_c, uint32_t *status) {
  Cfg c;
  if (cfg_from(cfg, c)) return -1;
  const ObsLayout L = obs_layout(c);
  const ContNet cross{Wc, mean_c, std_c}, wait{Ww, mean_w, std_w};
  const SampleNoise nz{eps, nullptr, key, first_env, t};
  const int S = c.nS;
  const uint32_t st = for_rows(M, [&](int64_t lo, int64_t hi) {
    uint32_t s = 0;
    for (int64_t r = lo; r < hi; r++)
      s |= sample_act_row(obs + r * L.obs_dim, L, cross, wait, a_d + r * S * c.P, closest + r * S, nz, r,
                          actions + r * 2 * S, act + r * S, logp + r * S, feat_c ? feat_c + r * S * NF_C : nullptr);
    return s;
  });
  if (status) *status |= st;
  return 0;
}

// the in-rule noise of rows [0, M) alone: u [M, S, P] and, for step t, eps [M, S] (either may be NULL)
int hp_sample_noise(const mhppo_env_cfg *cfg, int64_t M, uint64_t key, uint64_t first_env, int64_t t, float *u,
                    float *eps) {
  Cfg c;
  if (cfg_from(cfg, c)) return -1;
  const SampleNoise nz{nullptr, nullptr, key, first_env, t};
  const int SP = c.nS * c.P;
  if (u)
    for (int64_t q = 0; q < M * SP; q++) u[q] = noise_uniform(nz, q, SP);
  if (eps)
    for (int64_t k = 0; k < M * c.nS; k++) eps[k] = noise_normal(nz, k, c.nS);
  return 0;
}
}
