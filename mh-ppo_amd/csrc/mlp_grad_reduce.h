// mlp_grad_reduce.h — the deterministic (fixed order, float64) reductions of the train kernels'
// gradient partials into the packed float gradient and the three float64 sums (slot k < np is
// gradient k, slots np .. np + 2 the sums, which are ADDED to out3):
//   k_grad_reduce_blocks     the split kernels' float64 block partials (mlp_x3.h: one per block, at
//                            most one block per CU) in one launch; blockIdx.y = net of a pair launch
//   k_grad_stage1 / _stage2  the exact-f32 kernel's float partials, one per wave (mlp_train_f32.h):
//                            stage 1 sums RG contiguous groups of waves, stage 2 the RG group totals
// Part of the mlp_train.hip translation unit (one anonymous namespace); not for inclusion elsewhere.
#pragma once
#include <hip/hip_runtime.h>

namespace {
constexpr int RG = 64;

// blockIdx.z = net, for a launch that reduces two nets' partials at once (net z's partials follow
// net z - 1's in gpart / dpart; its group totals at tmp + z RG (np + 3)); the host launches one net.
template <class T>
__global__ void __launch_bounds__(256)
    k_grad_stage1(const T *gpart, const double *dpart, int nw, int np, double *tmp) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int g = blockIdx.y, nd = np + 3, z = blockIdx.z;
  gpart += (size_t)z * nw * np;
  dpart += (size_t)z * nw * 3;
  tmp += (size_t)z * RG * nd;
  const int i0 = (int)((int64_t)g * nw / RG), i1 = (int)((int64_t)(g + 1) * nw / RG);
  double s = 0.0;
  if (k < np) {
    // unrolled: the group's loads issue together (the sum order, and so the bits, unchanged)
#pragma unroll 16
    for (int i = i0; i < i1; i++) s += (double)gpart[(size_t)i * np + k];
  } else if (k < nd) {
    for (int i = i0; i < i1; i++) s += dpart[(size_t)i * 3 + (k - np)];
  } else {
    return;
  }
  tmp[(size_t)g * nd + k] = s;
}

// The split kernels' block partials (at most one per CU: nb <= 1024) in ONE launch: a 1 024-thread
// block per 64 gradient slots; thread (g, c) sums partials [g nb / 16, (g + 1) nb / 16) of slot c
// in order (16 coalesced rows per load step), then thread (0, c) adds the 16 group sums in order.
// blockIdx.y = net (the pair launch).  Fixed order: deterministic.
constexpr int RD_COLS = 64, RD_GROUPS = 16;
__global__ void __launch_bounds__(RD_COLS * RD_GROUPS)
    k_grad_reduce_blocks(const double *gpart, const double *dpart, int nb, int np, float *grad, double *out3,
                         float *grad1, double *out3_1) {
  __shared__ double red[RD_GROUPS][RD_COLS];
  const int c = blockIdx.x * RD_COLS + (threadIdx.x & (RD_COLS - 1)), g = threadIdx.x / RD_COLS;
  const int nd = np + 3;
  if (blockIdx.y) {
    gpart += (size_t)nb * np;
    dpart += (size_t)nb * 3;
    grad = grad1;
    out3 = out3_1;
  }
  const int i0 = g * nb / RD_GROUPS, i1 = (g + 1) * nb / RD_GROUPS;
  double s = 0.0;
  if (c < np) {
#pragma unroll 16
    for (int i = i0; i < i1; i++) s += gpart[(size_t)i * np + c];
  } else if (c < nd) {
    for (int i = i0; i < i1; i++) s += dpart[(size_t)i * 3 + (c - np)];
  }
  red[g][threadIdx.x & (RD_COLS - 1)] = s;
  __syncthreads();
  if (g != 0 || c >= nd) return;
  double t = 0.0;
#pragma unroll
  for (int q = 0; q < RD_GROUPS; q++) t += red[q][threadIdx.x];
  if (c < np)
    grad[c] = (float)t;
  else if (out3)
    out3[c - np] += t;
}

__global__ void __launch_bounds__(256)
    k_grad_stage2(const double *tmp, int np, float *grad, double *out3, float *grad1, double *out3_1) {
  const int k = blockIdx.x * 256 + threadIdx.x, nd = np + 3;
  if (k >= nd) return;
  if (blockIdx.z) {
    tmp += (size_t)RG * nd;
    grad = grad1;
    out3 = out3_1;
  }
  double s = 0.0;
#pragma unroll 8
  for (int g = 0; g < RG; g++) s += tmp[(size_t)g * nd + k];
  if (k < np)
    grad[k] = (float)s;
  else if (out3)
    out3[k - np] += s;
}
}  // namespace
