// common.h — what the libmhppo.so translation units share on the host side: error reporting, the
// device guard of an ABI call, the per-device scratch buffer, the cached CU count and the
// dynamic-LDS limit of a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <atomic>

namespace mhppo {
int set_error(int code, const char *fmt, ...);

// Makes `dev` the calling thread's current HIP device for the scope of one ABI call and
// restores the caller's device afterwards (a handle is bound to the device it was created
// on, include/mhppo.h; the caller's current device is never changed by a call).
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    int cur = -1;
    err = hipGetDevice(&cur);
    if (err == hipSuccess && cur != dev) {
      err = hipSetDevice(dev);
      if (err == hipSuccess) prev = cur;
    }
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
// per-device tables (workspaces, CU counts) hold this many devices
constexpr int MAX_DEVICES = 16;

// n doubles of device scratch on the current device, or nullptr (allocation failed, or a device
// number >= MAX_DEVICES).  ONE buffer per device, grown on demand (growing frees the old one) and
// shared by mhppo_rollout_begin's block counts and the loss entry points' block partials: every
// use is stream-ordered, and a call's contents mean nothing to the next.  (Hidden: the library's
// dynamic symbol list stays what it was.)
__attribute__((visibility("hidden"))) double *scratch(size_t n);

// The multiprocessor (CU) count of device `dev`, asked once per device (256 if the query fails; a
// device number outside the table is asked every time).
__attribute__((visibility("hidden"))) int device_cus(int dev);

// Dynamic LDS above the 64 KB a kernel gets by default: allow_dynamic_lds raises `kernel`'s limit
// on the current device to `bytes`, at most once per device and size (`limit`, one per kernel,
// static storage: what it was last raised to; a device number outside the table sets the attribute
// on every call).  MHPPO_OK, or the error already set.
struct LdsLimit {
  std::atomic<int> bytes[MAX_DEVICES];
};
__attribute__((visibility("hidden"))) int allow_dynamic_lds(const void *kernel, size_t bytes, LdsLimit &limit);
}  // namespace mhppo
using mhppo::set_error;

#define GUARD_DEVICE(dev)                                                                  \
  mhppo::DeviceGuard _dg(dev);                                                              \
  if (_dg.err != hipSuccess)                                                                \
    return set_error(MHPPO_EHIP, "hipSetDevice(%d) failed: %s", (int)(dev), hipGetErrorString(_dg.err))

#define CHECK_HIP(expr)                                                                     \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return set_error(MHPPO_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                       __FILE__, __LINE__);                                                 \
  } while (0)
