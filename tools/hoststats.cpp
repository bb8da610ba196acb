// hoststats.cpp — the streaming evaluation statistics on the CPU, from the device source:
// csrc/eval_stats_terms.h, the very row arithmetic eval_stats.hip runs, one env after another
// over a recorded trajectory, and the per-env accumulators folded in env order.  The CPU
// reference of tests/test_evalstats_host.py and tests/test_evalstats_gpu.py.
// Built with -ffp-contract=off -fno-builtin, as the device build's arithmetic.
// Build: make -C tools   ->  tools/libhoststats.so (ctypes, tools/hoststats.py)
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../mh-ppo_amd/csrc/eval_stats_terms.h"

using namespace mhppo;

extern "C" {
int hs_n(void) { return MHPPO_EVS_N; }

// traj float32 [K, T, E, obs_dim] (episode k, row t, env e) -> sums [MHPPO_EVS_N] and
// abs_sums [MHPPO_EVS_N] (the sum of |term| per entry).  -1: T < 2 or an unsupported layout.
int hs_stats(int variant, int slots, int nb_car, int nb_ped, int obs_dim, const float *traj, int64_t K, int64_t T,
             int64_t E, double *sums, double *abs_sums) {
  evs::Layout L;
  if (T < 2 || T > INT32_MAX || K < 0 || E < 0) return -1;
  if (!evs::layout(variant, slots, nb_car, nb_ped, obs_dim, L)) return -1;
  std::vector<double> state((evs::state_bytes(L, (size_t)E) + 7) / 8, 0.0);
  std::vector<double> abs_acc((size_t)MHPPO_EVS_N * E, 0.0);
  for (int64_t k = 0; k < K; k++)
    for (int64_t t = 0; t < T; t++)
      for (int64_t e = 0; e < E; e++) {
        evs::View<true> v(state.data(), abs_acc.data(), L, (size_t)E, (size_t)e);
        evs::row<true>(traj + ((k * T + t) * E + e) * obs_dim, L, (int)t, (int)T, v);
      }
  for (int j = 0; j < MHPPO_EVS_N; j++) {
    double s = 0.0, a = 0.0;
    for (int64_t e = 0; e < E; e++) {
      s += state[(size_t)j * E + e];
      a += abs_acc[(size_t)j * E + e];
    }
    sums[j] = s;
    abs_sums[j] = a;
  }
  return 0;
}
}
