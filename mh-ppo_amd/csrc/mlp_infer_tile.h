// mlp_infer_tile.h — one 32-row tile of a Model_PPO net (n_in <= 64 -> 32 -> 64 -> 32 -> 1 or 2) on
// f32 MFMA, forward only (device; mlp_infer.hip).
//
// The scheme of the rollout's 13 -> 1 actor tile (rollout_policy.h pol::actor_tile), generalised to
// a run-time input width and one or two outputs, on the same tile primitives and LDS row
// permutation (mfma_tile.h): C register r of lane half kh holds neuron 2 r + kh of the layer's
// output, so every chain runs in ascending input order.  The f32 MFMA is bit for bit a k-ordered
// fmaf chain (one rounding per product), so each output equals mlp_forward's (rollout_dev.h):
// ascending-k fmaf from 0, the bias added last.  Layer 1 runs ceil(n_in / 2) k-steps; an odd n_in
// is padded with a zero weight column and a zero input column (fmaf(0, 0, acc) == acc).
#pragma once
#include "mfma_tile.h"
#include "rollout_dev.h"

namespace mhppo {
namespace infer {
using namespace mfma_tile;  // f32x16, mfma, zero16, bias_relu, row_of_neuron, S2, S3

// LDS image of one net (floats).  S1: row stride of W1 and of a staged input tile: odd, and wide
// enough for the 2 ceil(n_in / 2) columns layer 1 reads.  The bias arrays start at multiples of 4
// floats (float4 reads).
struct Img {
  int S1, ks, o_b1, o_w2, o_b2, o_w3, o_b3, o_w4, o_b4, size;
};
__host__ __device__ inline Img img_layout(int n_in, int n_out) {
  Img g;
  g.S1 = (n_in & 1) ? n_in + 2 : n_in + 1;
  g.ks = (n_in + 1) / 2;
  g.o_b1 = 32 * g.S1;
  g.o_w2 = g.o_b1 + 32;
  g.o_b2 = g.o_w2 + 64 * S2;
  g.o_w3 = g.o_b2 + 64;
  g.o_b3 = g.o_w3 + 32 * S3;
  g.o_w4 = g.o_b3 + 32;
  g.o_b4 = g.o_w4 + 32 * n_out;
  g.size = (g.o_b4 + n_out + 3) / 4 * 4;
  return g;
}
__host__ __device__ inline int xtile_floats(const Img &g) { return (32 * g.S1 + 3) / 4 * 4; }
// 32-row tiles of M rows
inline int64_t n_tiles(int64_t M) { return (M + 31) / 32; }

// One torch-packed net (W1 b1 W2 b2 W3 b3 W4 b4) into its LDS image: the rows of W1 / W2 / W3 and
// the entries of b1 / b2 / b3 at the permuted row of their neuron, W1's padding columns zeroed.
// Coalesced source-order reads; the caller synchronises the block afterwards.
template <int NT>
__device__ __forceinline__ void stage_image(float *L, const Img &g, const float *__restrict__ W, int n_in, int n_out,
                                            int tid) {
  const int nw1 = 32 * n_in;
  const float *b1 = W + nw1, *w2 = b1 + 32, *b2 = w2 + 2048, *w3 = b2 + 64, *b3 = w3 + 2048, *w4 = b3 + 32,
              *b4 = w4 + 32 * n_out;
#pragma unroll 2
  for (int x = tid; x < nw1; x += NT) {
    const int n = x / n_in, k = x - n * n_in;
    L[row_of_neuron(n) * g.S1 + k] = W[x];
  }
  const int pad = g.S1 - n_in;  // 1 or 2 padding columns per row
#pragma unroll 1
  for (int x = tid; x < 32 * pad; x += NT) L[(x / pad) * g.S1 + n_in + x % pad] = 0.0f;
  for (int x = tid; x < 2048; x += NT) {
    const int n2 = x >> 5, k2 = x & 31;  // W2 [64][32]
    L[g.o_w2 + ((n2 & 32) + row_of_neuron(n2 & 31)) * S2 + k2] = w2[x];
    const int n3 = x >> 6, k3 = x & 63;  // W3 [32][64]
    L[g.o_w3 + row_of_neuron(n3) * S3 + k3] = w3[x];
  }
  if (tid < 32) {
    L[g.o_b1 + row_of_neuron(tid)] = b1[tid];
    L[g.o_b3 + row_of_neuron(tid)] = b3[tid];
  }
  if (tid < 64) L[g.o_b2 + (tid & 32) + row_of_neuron(tid & 31)] = b2[tid];
#pragma unroll 1
  for (int x = tid; x < 32 * n_out; x += NT) L[g.o_w4 + x] = w4[x];
  if (tid < n_out) L[g.o_b4 + tid] = b4[tid];
}

// A wave's staged input tile xs [32][S1] from X rows [r0, r0 + nr): the nr * n_in floats are one
// contiguous run, read 64 lanes at a time (a row-per-lane read of n_in-float rows is not
// coalesced).  (row, col) of the lane's q-th element advance by 64 / n_in rows and 64 % n_in
// columns per step (st_row, st_col): no division per element.  Rows >= nr are zeroed.
struct XStage {
  int row0, col0, st_row, st_col;  // the lane's first element; the per-step advance
};
__device__ __forceinline__ XStage xstage_init(int n_in, int lane) {
  XStage s;
  s.row0 = lane / n_in;
  s.col0 = lane - s.row0 * n_in;
  s.st_row = 64 / n_in;
  s.st_col = 64 - s.st_row * n_in;
  return s;
}
__device__ __forceinline__ void stage_x(float *xs, const Img &g, const XStage &s, const float *__restrict__ X,
                                        int64_t r0, int nr, int n_in, int lane) {
  const float *src = X + r0 * n_in;
  const int n = nr * n_in, tot = 32 * n_in;
  int row = s.row0, col = s.col0;
  // eight loads in flight per lane, then their stores (13 inputs: one batch of 7)
#pragma unroll 1
  for (int e0 = lane; e0 < tot; e0 += 8 * 64) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int e = e0 + 64 * q;
      v[q] = e < n ? src[e] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < 8; q++) {
      if (e0 + 64 * q < tot) xs[row * g.S1 + col] = v[q];
      row += s.st_row;
      col += s.st_col;
      if (col >= n_in) {
        col -= n_in;
        row++;
      }
    }
  }
}
// stage_x in two halves, for a tile prefetched behind another tile's MFMA chain (mlp_gae.hip):
// stage_x_issue starts the loads of the lane's first eight elements (every element of a tile of up
// to 16 inputs) into registers, stage_x_land stores them to xs and stages what is left as stage_x
// does.  src = X + r0 * n_in, the tile's first element.
__device__ __forceinline__ void stage_x_issue(float (&pre)[8], const float *__restrict__ src, int nr, int n_in,
                                              int lane) {
  const int n = nr * n_in;
#pragma unroll
  for (int q = 0; q < 8; q++) {
    const int e = lane + 64 * q;
    pre[q] = e < n ? src[e] : 0.0f;
  }
}
__device__ __forceinline__ void stage_x_land(float *xs, const Img &g, const XStage &s, const float (&pre)[8],
                                             const float *__restrict__ src, int nr, int n_in, int lane) {
  const int n = nr * n_in, tot = 32 * n_in;
  int row = s.row0, col = s.col0;
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; q++) v[q] = pre[q];
#pragma unroll 1
  for (int e0 = lane;;) {
#pragma unroll
    for (int q = 0; q < 8; q++) {
      if (e0 + 64 * q < tot) xs[row * g.S1 + col] = v[q];
      row += s.st_row;
      col += s.st_col;
      if (col >= n_in) {
        col -= n_in;
        row++;
      }
    }
    e0 += 8 * 64;
    if (e0 >= tot) break;
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const int e = e0 + 64 * q;
      v[q] = e < n ? src[e] : 0.0f;
    }
  }
}
// zero the padding columns of a staged input tile (once: stage_x never writes them)
__device__ __forceinline__ void zero_x_pad(float *xs, const Img &g, int n_in, int lane) {
  const int pad = g.S1 - n_in;
#pragma unroll 1
  for (int x = lane; x < 32 * pad; x += 64) xs[(x / pad) * g.S1 + n_in + x % pad] = 0.0f;
}

// One 32-row tile through one net (Wl: its LDS image; xs: the wave's staged inputs): z[o] = output o
// of tile row j before the head's finish, in every lane of both halves.
// Layers 2-4 are the chain of pol::actor_tile (rollout_policy.h) with this image's run-time offsets:
// change the two together.  (No form of one shared function left both these kernels' instruction
// streams and k_policy_mfma's as they were: profiles/rollout_split/kernels.txt.)
template <int NOUT>
__device__ __forceinline__ void tile_forward(const float *Wl, const Img &g, const float *xs, int j, int kh,
                                             float (&z)[NOUT]) {
  f32x16 h1 = zero16();
  {
    const float *wr = Wl + j * g.S1 + kh, *xr = xs + j * g.S1 + kh;
    for (int s = 0; s < g.ks; s++) h1 = mfma(wr[2 * s], xr[2 * s], h1);
  }
  bias_relu(h1, Wl + g.o_b1, kh);
  f32x16 h2a = zero16(), h2b = zero16();
  const float *w2 = Wl + g.o_w2 + kh;
#pragma unroll
  for (int s = 0; s < 16; s++) {
    h2a = mfma(w2[j * S2 + 2 * s], h1[s], h2a);
    h2b = mfma(w2[(32 + j) * S2 + 2 * s], h1[s], h2b);
  }
  bias_relu(h2a, Wl + g.o_b2, kh);
  bias_relu(h2b, Wl + g.o_b2 + 32, kh);
  f32x16 h3 = zero16();
  const float *w3 = Wl + g.o_w3 + j * S3 + kh;
#pragma unroll
  for (int s = 0; s < 16; s++) h3 = mfma(w3[2 * s], h2a[s], h3);
#pragma unroll
  for (int s = 0; s < 16; s++) h3 = mfma(w3[32 + 2 * s], h2b[s], h3);
  bias_relu(h3, Wl + g.o_b3, kh);
  float y[NOUT];
#pragma unroll
  for (int o = 0; o < NOUT; o++) y[o] = 0.0f;
  const float *w4 = Wl + g.o_w4;
#pragma unroll
  for (int s = 0; s < 16; s++) {
    // neuron 2s sits in register s of the lower lane half, 2s + 1 in the upper: one
    // v_permlane32_swap gives every lane both (r[0] = neuron 2s, r[1] = neuron 2s + 1 of its row)
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(h3[s]), __float_as_uint(h3[s]), false, false);
#pragma unroll
    for (int o = 0; o < NOUT; o++) {
      y[o] = fmaf(w4[32 * o + 2 * s], __uint_as_float(r[0]), y[o]);
      y[o] = fmaf(w4[32 * o + 2 * s + 1], __uint_as_float(r[1]), y[o]);
    }
  }
#pragma unroll
  for (int o = 0; o < NOUT; o++) z[o] = y[o] + Wl[g.o_b4 + o];
}

}  // namespace infer
}  // namespace mhppo
