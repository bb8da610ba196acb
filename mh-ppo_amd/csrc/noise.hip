// noise.hip — counter-based noise and the libm pin (+ C-ABI): Philox-4x32-10 uniforms and
// Box-Muller normals keyed by (seed, counter), so a draw depends on its index alone
// (mhppo_philox_uniform / _normal / _normal_2d: the rollout's choice uniforms and MVN noise), and
// the device side of the exhaustive pin of the policy heads' glibc-exact transcendentals
// (mhppo_libm_eval).
#include <hip/hip_runtime.h>

#include "../../include/mhppo.h"
#include "common.h"
#include "launch1d.h"
#include "libm_glibc.h"
#include "ppo_math.h"  // philox_draw

using namespace mhppo;

namespace {

__global__ void __launch_bounds__(TPB) k_philox(uint64_t seed, uint64_t off, float *out, int64_t n, int normal) {
  int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  out[i] = philox_draw(seed, off + (uint64_t)i, normal != 0);
}

// The policy heads' glibc-exact transcendentals (libm_glibc.h) over float bit patterns
// first .. first + n - 1 (mod 2^32): the device side of their exhaustive pin (mhppo_libm_eval)
__global__ void __launch_bounds__(TPB) k_libm_eval(int fn, uint64_t first, int64_t n, float *out) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const float x = __uint_as_float((uint32_t)(first + (uint64_t)i));
  out[i] = fn == 0 ? mhppo_tanhf(x) : (fn == 1 ? mhppo_expm1f(x) : mhppo_expf(x));
}

// rows x cols standard normals, element (r, c) from counter off + r * stride + c (one
// launch for a whole rollout's per-step MVN noise: bit-identical to `rows` 1-D calls)
__global__ void __launch_bounds__(TPB) k_philox_normal_2d(uint64_t seed, uint64_t off, uint64_t stride, float *out,
                                                          int64_t rows, int64_t cols) {
  const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= rows * cols) return;
  const int64_t r = i / cols, cc = i - r * cols;
  const uint64_t ctr = off + (uint64_t)r * stride + (uint64_t)cc;
  out[i] = philox_draw(seed, ctr, true);
}

}  // namespace

extern "C" {

int mhppo_philox_normal(uint64_t seed, uint64_t offset, float *out, int64_t n, void *stream) {
  if (!out || n < 0) return set_error(MHPPO_EINVAL, "bad argument");
  if (n == 0) return MHPPO_OK;
  hipLaunchKernelGGL(k_philox, grid_for(n), dim3(TPB), 0, (hipStream_t)stream, seed, offset, out, n, 1);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_philox_normal_2d(uint64_t seed, uint64_t offset, uint64_t stride, float *out, int64_t rows, int64_t cols,
                           void *stream) {
  if (!out || rows < 0 || cols < 0) return set_error(MHPPO_EINVAL, "bad argument");
  if (rows == 0 || cols == 0) return MHPPO_OK;
  hipLaunchKernelGGL(k_philox_normal_2d, grid_for((size_t)(rows * cols)), dim3(TPB), 0, (hipStream_t)stream, seed,
                     offset, stride, out, rows, cols);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_philox_uniform(uint64_t seed, uint64_t offset, float *out, int64_t n, void *stream) {
  if (!out || n < 0) return set_error(MHPPO_EINVAL, "bad argument");
  if (n == 0) return MHPPO_OK;
  hipLaunchKernelGGL(k_philox, grid_for(n), dim3(TPB), 0, (hipStream_t)stream, seed, offset, out, n, 0);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_libm_eval(int fn, uint64_t first, int64_t n, float *out, void *stream) {
  if (!out || n < 0 || fn < 0 || fn > 2) return set_error(MHPPO_EINVAL, "bad argument (fn 0 tanhf, 1 expm1f, 2 expf)");
  if (n == 0) return MHPPO_OK;
  hipLaunchKernelGGL(k_libm_eval, grid_for(n), dim3(TPB), 0, (hipStream_t)stream, fn, first, n, out);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

}  // extern "C"
