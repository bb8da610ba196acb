// eval_stats.hip — streaming evaluation statistics (+ C-ABI): get_average's sums without a
// trajectory (include/mhppo.h MHPPO_EVS_*; the arithmetic is eval_stats_terms.h, shared with the
// host harness tools/hoststats.cpp).
//   k_evs_row   one lane per env: the env's observation row -> its carry and float64 accumulators.
//               The row read is the hot part (N * obs_dim floats per step).  The columns used are
//               about half of a 96-200 B row that starts at no line boundary, so a per-column read
//               would fetch every line anyway, 64 lines per load instruction; instead a block copies
//               its envs' rows — one contiguous run of floats — into LDS with coalesced loads and
//               each lane reads its row from there (row stride odd: conflict-free).
//   k_evs_fold  one block per sum: the per-env accumulators of that sum folded in the fixed
//               order of block_prims.h (k_fold: 1024 threads, four chains per thread, then the
//               tree), written — not added — to sums.
#include <hip/hip_runtime.h>

#include "../../include/mhppo.h"
#include "block_prims.h"
#include "common.h"
#include "eval_stats_terms.h"

using namespace mhppo;

namespace mhppo {
const Cfg &env_cfg(const mhppo_env *env);
int env_device(const mhppo_env *env);
}  // namespace mhppo

namespace {
constexpr int ROW_TPB = 128;
constexpr int FOLD_TPB = 1024;
constexpr size_t ROW_LDS_MAX = 64 * 1024;

__host__ __device__ inline int row_stride(int obs_dim) { return obs_dim | 1; }

__global__ void __launch_bounds__(ROW_TPB)
    k_evs_row(evs::Layout L, int N, const float *__restrict__ obs, int t, int T, void *state) {
  extern __shared__ float s_rows[];
  const int od = L.obs_dim, rs = row_stride(od);
  const int e0 = blockIdx.x * ROW_TPB;
  const int ne = min(ROW_TPB, N - e0);
  const float *src = obs + (size_t)e0 * od;
  for (int k = threadIdx.x; k < ne * od; k += ROW_TPB) {
    const int r = k / od;
    s_rows[r * rs + (k - r * od)] = src[k];
  }
  __syncthreads();
  if ((int)threadIdx.x >= ne) return;
  evs::View<false> v(state, nullptr, L, (size_t)N, (size_t)(e0 + threadIdx.x));
  evs::row<false>(s_rows + threadIdx.x * rs, L, t, T, v);
}

constexpr auto k_evs_fold = k_fold<FOLD_TPB, 4, false>;

int env_layout(const mhppo_env *env, evs::Layout &L) {
  const Cfg &c = env_cfg(env);
  if (!evs::layout(c.variant, c.nS, c.nb_car, c.P, c.obs_dim, L))
    return set_error(MHPPO_EINVAL, "the evaluation statistics are defined for the scalable/coop/naif/stop "
                     "observation layout (car|env|ped) with nb_car <= car slots, not variant %d (nb_car %d, %d slots)",
                     c.variant, c.nb_car, c.nS);
  return MHPPO_OK;
}
}  // namespace

extern "C" {

int64_t mhppo_eval_stats_bytes(const mhppo_env *env) {
  if (!env) return set_error(MHPPO_EINVAL, "null argument");
  evs::Layout L;
  int rc = env_layout(env, L);
  if (rc) return rc;
  return (int64_t)evs::state_bytes(L, (size_t)env_cfg(env).N);
}

int mhppo_eval_stats_begin(mhppo_env *env, void *state, void *stream) {
  if (!env || !state) return set_error(MHPPO_EINVAL, "null argument");
  evs::Layout L;
  int rc = env_layout(env, L);
  if (rc) return rc;
  GUARD_DEVICE(env_device(env));
  CHECK_HIP(hipMemsetAsync(state, 0, evs::state_bytes(L, (size_t)env_cfg(env).N), (hipStream_t)stream));
  return MHPPO_OK;
}

int mhppo_eval_stats_row(mhppo_env *env, const float *obs, int t, int T, void *state, void *stream) {
  if (!env || !obs || !state) return set_error(MHPPO_EINVAL, "null argument");
  if (T < 2) return set_error(MHPPO_EINVAL, "an episode needs at least two rows (T = %d)", T);
  if (t < 0 || t >= T) return set_error(MHPPO_EINVAL, "row %d outside [0, %d)", t, T);
  evs::Layout L;
  int rc = env_layout(env, L);
  if (rc) return rc;
  const Cfg &c = env_cfg(env);
  const size_t shm = sizeof(float) * ROW_TPB * row_stride(c.obs_dim);
  if (shm > ROW_LDS_MAX) return set_error(MHPPO_EINVAL, "observation rows of %d floats: row staging needs %zu B of LDS", c.obs_dim, shm);
  if (c.N <= 0) return MHPPO_OK;
  GUARD_DEVICE(env_device(env));
  const unsigned grid = (unsigned)((c.N + ROW_TPB - 1) / ROW_TPB);
  hipLaunchKernelGGL(k_evs_row, dim3(grid), dim3(ROW_TPB), shm, (hipStream_t)stream, L, c.N, obs, t, T, state);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_eval_stats_fold(mhppo_env *env, const void *state, double *sums, void *stream) {
  if (!env || !state || !sums) return set_error(MHPPO_EINVAL, "null argument");
  evs::Layout L;
  int rc = env_layout(env, L);
  if (rc) return rc;
  GUARD_DEVICE(env_device(env));
  hipLaunchKernelGGL(k_evs_fold, dim3(MHPPO_EVS_N), dim3(FOLD_TPB), 0, (hipStream_t)stream,
                     static_cast<const double *>(state), env_cfg(env).N, sums);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

}  // extern "C"
