// mlp_train.hip — the train translation unit: one fused forward + loss gradient + backward +
// weight gradient pass of a Model_PPO head per call (mhppo_mlp_train), or the continuous actor's
// pass fused with the next epoch's critic pass (mhppo_mlp_train_pair).  This file holds the host
// side: the per-stream partial buffers (Work), the choice of kernel for (kind, n_in), the launches
// and the C ABI.  The kernels are in the headers below, one per family, all in this TU's anonymous
// namespace (they are built with this file's flags, csrc/Makefile):
//   mlp_tile.h         what both families share: kinds, LDS input slots, tile loaders
//   mlp_train_f32.h    the exact-f32 kernel k_mlp_train (MHPPO_TRAIN_EXACT_F32, n_in > 54)
//   mlp_x3_prims.h     the split-precision (bf16x3) primitives
//   mlp_x3.h           the split-precision kernels k_mlp_train_x3 / k_mlp_train_x3_pair (the default)
//   mlp_grad_reduce.h  the reductions of the kernels' gradient partials
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/mhppo.h"
#include "common.h"
// (this order is the order of the kernels in the code object)
#include "mlp_tile.h"
#include "mlp_train_f32.h"
#include "mlp_x3_prims.h"
#include "mlp_x3.h"
#include "mlp_grad_reduce.h"

namespace {
// Per-stream partial buffers: g the kernels' gradient partials, d their float64 sums (three per
// partial), t the f32 path's stage-1 group totals.  Sized for `nw` wave slots of the widest net.
struct Work {
  float *g = nullptr;
  double *d = nullptr;
  double *t = nullptr;
  int nw = 0;
  // The split kernels write ONE float64 partial per block (np <= NW_MAX doubles each), not a float
  // one per wave: a launch of `blocks` blocks per net has blocks * WAVES slots per net, i.e.
  // blocks * WAVES * NW_MAX floats, which hold blocks * NW_MAX doubles as long as WAVES floats are
  // at least one double (hipMalloc's alignment covers the doubles').
  double *g64() const {
    static_assert(x3::WAVES * sizeof(float) >= sizeof(double), "a block's wave slots hold its float64 partial");
    return reinterpret_cast<double *>(g);
  }
};
// per device and stream (up to WORK_STREAMS streams per device may run train passes concurrently:
// each stream's passes reduce through their own partial buffers; calls on one stream are ordered)
constexpr int WORK_STREAMS = 4;
Work g_work[mhppo::MAX_DEVICES][WORK_STREAMS];
hipStream_t g_work_stream[mhppo::MAX_DEVICES][WORK_STREAMS];
int g_work_used[mhppo::MAX_DEVICES] = {0};
// partial buffers for `slots` waves' partials (a fused pair launch uses two slots per wave)
bool ensure_work(Work &wk, int slots) {
  if (wk.nw >= slots) return true;
  if (wk.g) (void)hipFree(wk.g);
  if (wk.d) (void)hipFree(wk.d);
  if (wk.t) (void)hipFree(wk.t);
  if (hipMalloc(&wk.g, sizeof(float) * (size_t)slots * NW_MAX) != hipSuccess ||
      hipMalloc(&wk.d, sizeof(double) * (size_t)slots * 3) != hipSuccess ||
      hipMalloc(&wk.t, sizeof(double) * (size_t)2 * RG * (NW_MAX + 3)) != hipSuccess) {
    wk = Work{};
    return false;
  }
  wk.nw = slots;
  return true;
}
Work *device_work(int dev, hipStream_t s) {
  int k = 0;
  while (k < g_work_used[dev] && g_work_stream[dev][k] != s) k++;
  if (k == g_work_used[dev]) {
    if (k == WORK_STREAMS) return nullptr;
    g_work_stream[dev][k] = s;
    g_work_used[dev] = k + 1;
  }
  return &g_work[dev][k];
}

// What a launch needs besides its arguments: the stream's partial buffers and the grid (one block
// per CU at most, grid-stride over 32-row tiles; nw = the wave slots of one net).
struct Launch {
  Work *wk;
  int blocks, nw;
};
// When X's 16-byte alignment (its rows are read by LDS-DMA) is checked: the 13-input heads check it
// before the stream lookup, the choice heads on the split kernel after it.  The order in which a
// call's errors fire is part of the ABI's behaviour, so both stay where they were.
enum XAlign { X_ANY, X_16B_BEFORE_LOOKUP, X_16B_AFTER_LOOKUP };
// The checks and preparation shared by the entry points, for M > 0 rows: M's upper bound, X's
// alignment, the current device's per-stream Work, the grid for `waves` waves per block, and the
// partial buffers for `nets` nets.  MHPPO_OK, or the error already set.
int prepare_launch(hipStream_t s, int64_t M, const float *X, XAlign xa, int waves, int nets, Launch &L) {
  if (M > ((int64_t)1 << 40)) return set_error(MHPPO_EINVAL, "M too large");
  const bool misaligned = ((uintptr_t)X & 15) != 0;
  if (xa == X_16B_BEFORE_LOOKUP && misaligned)
    return set_error(MHPPO_EINVAL, "X must be 16-byte aligned (LDS-DMA rows)");
  int dev = 0;
  CHECK_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= mhppo::MAX_DEVICES) return set_error(MHPPO_EINVAL, "device %d >= %d", dev, mhppo::MAX_DEVICES);
  L.wk = device_work(dev, s);
  if (!L.wk) return set_error(MHPPO_EINVAL, "train passes on more than %d streams of one device", WORK_STREAMS);
  if (xa == X_16B_AFTER_LOOKUP && misaligned)
    return set_error(MHPPO_EINVAL, "X must be 16-byte aligned (LDS-DMA rows)");
  const int64_t tiles = (M + 31) / 32;
  L.blocks = (int)std::max<int64_t>(1, std::min<int64_t>(mhppo::device_cus(dev), (tiles + waves - 1) / waves));
  L.nw = L.blocks * waves;
  if (!ensure_work(*L.wk, nets * L.nw)) return set_error(MHPPO_ENOMEM, "mlp_train partials");
  return MHPPO_OK;
}

// The split-precision instantiation for a head: the 13-input critic / continuous actor on the
// hand-placed geometry, a choice head's nets (n_in <= NIN_X3C) on the smallest layer-1 K that takes
// the inputs and the bias column (54 inputs: the compile-time count).
using X3Kernel = decltype(&k_mlp_train_x3<K_CRITIC, x3::G13S>);
struct X3Launch {
  X3Kernel kernel;
  int lds_bytes;
};
template <int KIND, class G>
constexpr X3Launch x3_of() { return {k_mlp_train_x3<KIND, G>, G::LDS_BYTES}; }
X3Launch x3_kernel(int kind, int n_in) {
  using namespace x3;
  const bool critic = kind == K_CRITIC;
  if (n_in == NIN_CONT && kind != K_CHOICE) return critic ? x3_of<K_CRITIC, G13S>() : x3_of<K_CONT, G13S>();
  if (n_in <= 15) return critic ? x3_of<K_CRITIC, GV16>() : x3_of<K_CHOICE, GC16>();
  if (n_in <= 31) return critic ? x3_of<K_CRITIC, GV32>() : x3_of<K_CHOICE, GC32>();
  if (n_in == 54) return critic ? x3_of<K_CRITIC, GV54>() : x3_of<K_CHOICE, GC54>();
  return critic ? x3_of<K_CRITIC, GV64>() : x3_of<K_CHOICE, GC64>();
}
// The exact-f32 instantiation for a head: the 13-input heads on the prefetching kernel, the others
// by their layer-1 k-steps KS (the inputs padded to 2 KS columns).
using F32Launch = decltype(&launch<K_CRITIC, 7, true>);
F32Launch f32_launcher(int kind, int n_in) {
  if (n_in == NIN_CONT && kind != K_CHOICE)
    return kind == K_CRITIC ? launch<K_CRITIC, 7, true> : launch<K_CONT, 7, true>;
  static constexpr F32Launch CRITIC[6] = {launch<K_CRITIC, 8, false>,  launch<K_CRITIC, 12, false>,
                                          launch<K_CRITIC, 16, false>, launch<K_CRITIC, 24, false>,
                                          launch<K_CRITIC, 28, false>, launch<K_CRITIC, 32, false>};
  static constexpr F32Launch CHOICE[6] = {launch<K_CHOICE, 8, false>,  launch<K_CHOICE, 12, false>,
                                          launch<K_CHOICE, 16, false>, launch<K_CHOICE, 24, false>,
                                          launch<K_CHOICE, 28, false>, launch<K_CHOICE, 32, false>};
  const int w = n_in <= 16 ? 0 : (n_in <= 24 ? 1 : (n_in <= 32 ? 2 : (n_in <= 48 ? 3 : (n_in <= 56 ? 4 : 5))));
  return (kind == K_CRITIC ? CRITIC : CHOICE)[w];
}
}  // namespace

#ifdef MHPPO_TIMING
// A/B timing builds only (not in include/mhppo.h): copy out and clear this TU's g_timing
extern "C" int mhppo_debug_timing_train(unsigned long long *out16) {
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_timing), sizeof(unsigned long long) * 16));
  unsigned long long z[16] = {0};
  CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_timing), z, sizeof(z)));
  return MHPPO_OK;
}
#endif

extern "C" int mhppo_mlp_train(int kind, int n_in, const float *packed, const float *X, int64_t M, const float *ret,
                               float *value, const float *act, const float *logp_old, const double *stats,
                               const double *counts, double m_global, float out_mean, float out_std, float *grad,
                               double *sums, void *stream) {
  const bool exact = (kind & MHPPO_TRAIN_EXACT_F32) != 0;
  kind &= ~MHPPO_TRAIN_EXACT_F32;
  if (!grad || M < 0 || kind < K_CRITIC || kind > K_CHOICE || n_in < 1 || n_in > NIN_MAX)
    return set_error(MHPPO_EINVAL, "bad argument (kind 0..2 [| MHPPO_TRAIN_EXACT_F32], 1 <= n_in <= %d)", NIN_MAX);
  hipStream_t s = (hipStream_t)stream;
  const int np = n_params(n_in, kind == K_CHOICE ? 2 : 1);
  if (M == 0) {  // an empty shard (data parallel): zero gradient, sums unchanged; X/ret/value may be NULL
    CHECK_HIP(hipMemsetAsync(grad, 0, sizeof(float) * np, s));
    return MHPPO_OK;
  }
  if (!packed || !X || !ret || !value) return set_error(MHPPO_EINVAL, "null packed/X/ret/value");
  if (kind == K_CONT && (n_in != NIN_CONT || !act || !logp_old || !stats))
    return set_error(MHPPO_EINVAL, "continuous actor pass needs n_in 13 and act/logp_old/stats");
  if (kind == K_CHOICE && (!logp_old || !stats || (!counts && !act)))
    return set_error(MHPPO_EINVAL, "choice actor pass needs logp_old/stats and counts (or act for per-row mode)");
  const bool pf = n_in == NIN_CONT && kind != K_CHOICE;  // the 13-input heads: LDS-DMA prefetch on either kernel
  // the split-precision kernel: the default for the 13-input heads and for the choice heads' nets of
  // up to NIN_X3C inputs (wider ones: f32 MFMA)
  const bool split = !exact && (pf || n_in <= x3::NIN_X3C);
  const int waves = split ? x3::WAVES : (pf ? 8 : 4);
  Launch L;
  const int rc = prepare_launch(s, M, X, pf ? X_16B_BEFORE_LOOKUP : (split ? X_16B_AFTER_LOOKUP : X_ANY), waves, 1, L);
  if (rc != MHPPO_OK) return rc;
  Work &wk = *L.wk;
  const dim3 grid((unsigned)L.blocks);
  if (split) {  // one float64 partial per block: one reduction launch
    const X3Launch k = x3_kernel(kind, n_in);
    hipLaunchKernelGGL(k.kernel, grid, dim3(64 * x3::WAVES), k.lds_bytes, s, packed, X, n_in, M, ret, value, act,
                       logp_old, stats, counts, m_global, out_mean, out_std, wk.g64(), wk.d);
    hipLaunchKernelGGL(k_grad_reduce_blocks, dim3((np + 3 + RD_COLS - 1) / RD_COLS), dim3(RD_COLS * RD_GROUPS), 0, s,
                       wk.g64(), wk.d, L.blocks, np, grad, sums, nullptr, nullptr);
  } else {  // one float partial per wave: two stages
    f32_launcher(kind, n_in)(grid, s, packed, X, n_in, M, ret, value, act, logp_old, stats, counts, m_global, out_mean,
                             out_std, wk.g, wk.d);
    hipLaunchKernelGGL(k_grad_stage1<float>, dim3((np + 3 + 255) / 256, RG), dim3(256), 0, s, wk.g, wk.d, L.nw, np,
                       wk.t);
    hipLaunchKernelGGL(k_grad_stage2, dim3((np + 3 + 255) / 256), dim3(256), 0, s, wk.t, np, grad, sums, nullptr,
                       nullptr);
  }
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

extern "C" int mhppo_mlp_train_pair(const float *packed_actor, const float *packed_critic, const float *X, int64_t M,
                                    const float *ret, float *value, const float *act, const float *logp_old,
                                    const double *stats, double m_global, float out_mean, float out_std,
                                    float *grad_actor, double *sums_actor, float *grad_critic, double *sums_critic,
                                    void *stream) {
  if (!grad_actor || !grad_critic || M < 0) return set_error(MHPPO_EINVAL, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int np = n_params(NIN_CONT, 1);
  if (M == 0) {  // an empty shard: zero gradients, sums unchanged
    CHECK_HIP(hipMemsetAsync(grad_actor, 0, sizeof(float) * np, s));
    CHECK_HIP(hipMemsetAsync(grad_critic, 0, sizeof(float) * np, s));
    return MHPPO_OK;
  }
  if (!packed_actor || !packed_critic || !X || !ret || !value || !act || !logp_old || !stats)
    return set_error(MHPPO_EINVAL, "null pointer");
  Launch L;
  const int rc = prepare_launch(s, M, X, X_16B_BEFORE_LOOKUP, x3::WAVES, 2, L);
  if (rc != MHPPO_OK) return rc;
  Work &wk = *L.wk;
  hipLaunchKernelGGL(k_mlp_train_x3_pair, dim3((unsigned)L.blocks), dim3(64 * x3::WAVES), x3::G13::LDS_BYTES_PAIR, s,
                     packed_actor, packed_critic, X, M, ret, value, act, logp_old, stats, m_global, out_mean, out_std,
                     wk.g64(), wk.d);
  // the two nets' block partials (actor [0, blocks), critic [blocks, 2 blocks)) in one launch
  hipLaunchKernelGGL(k_grad_reduce_blocks, dim3((np + 3 + RD_COLS - 1) / RD_COLS, 2), dim3(RD_COLS * RD_GROUPS), 0, s,
                     wk.g64(), wk.d, L.blocks, np, grad_actor, sums_actor, grad_critic, sums_critic);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}
