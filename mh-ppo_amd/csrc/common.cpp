// common.cpp — thread-local last-error message, version string and the per-device scratch buffer.
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
}  // namespace mhppo

extern "C" const char *mhppo_last_error(void) { return mhppo::g_err; }
extern "C" const char *mhppo_version(void) { return "mhppo-mi355x 0.1 gfx950"; }
