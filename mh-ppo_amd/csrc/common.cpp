// common.cpp — thread-local last-error message, version string, the per-device scratch buffer, the
// cached CU counts and the dynamic-LDS limits.
#include <stdarg.h>
#include <stdio.h>

#include "../../include/mhppo.h"
#include "common.h"

namespace mhppo {
static thread_local char g_err[512] = "";
int set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

// scratch for partial sums (per device, grown on demand, stream-ordered use)
namespace {
struct Scratch {
  double *p = nullptr;
  size_t n = 0;
};
Scratch g_scratch[MAX_DEVICES];
}  // namespace

double *scratch(size_t n) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return nullptr;
  Scratch &s = g_scratch[dev];
  if (s.n < n) {
    if (s.p) (void)hipFree(s.p);
    if (hipMalloc(&s.p, n * sizeof(double)) != hipSuccess) {
      s.p = nullptr;
      s.n = 0;
      return nullptr;
    }
    s.n = n;
  }
  return s.p;
}

int device_cus(int dev) {
  static std::atomic<int> cus[MAX_DEVICES];
  const bool tracked = dev >= 0 && dev < MAX_DEVICES;
  if (tracked)
    if (const int n = cus[dev].load(std::memory_order_relaxed)) return n;
  int n = 256;
  (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
  if (tracked) cus[dev].store(n, std::memory_order_relaxed);
  return n;
}

int allow_dynamic_lds(const void *kernel, size_t bytes, LdsLimit &limit) {
  if (bytes <= 64 * 1024) return MHPPO_OK;
  int dev = -1;
  CHECK_HIP(hipGetDevice(&dev));
  const bool tracked = dev >= 0 && dev < MAX_DEVICES;
  if (tracked && limit.bytes[dev].load(std::memory_order_relaxed) >= (int)bytes) return MHPPO_OK;
  CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if (tracked) limit.bytes[dev].store((int)bytes, std::memory_order_relaxed);
  return MHPPO_OK;
}
}  // namespace mhppo

extern "C" const char *mhppo_last_error(void) { return mhppo::g_err; }
extern "C" const char *mhppo_version(void) { return "mhppo-mi355x 0.1 gfx950"; }
