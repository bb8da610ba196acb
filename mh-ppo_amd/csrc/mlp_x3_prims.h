// mlp_x3_prims.h — the building blocks of the split-precision (bf16x3) train kernel, mlp_x3.h.
// Every GEMM of that kernel runs on bf16 MFMA (v_mfma_f32_32x32x16_bf16: 16x the f32-MFMA
// rate) with each f32 operand split EXACTLY into three bf16 parts, x = hi + mid + lo
// (round-to-nearest at each level: |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|), and the six
// products of combined order <= 2 accumulated in f32: the dropped terms are <= 2^-24
// relative, i.e. the accuracy of an f32 product (the f32-MFMA kernel, mlp_train_f32.h, stays the
// exact k-ordered-fmaf reference, MHPPO_TRAIN_EXACT_F32).
// Orientation as there (activations transposed, C registers of one layer = B operand of
// the next with the permuted k order feature(16s + 8(j>>2) + 4h + (j&3)) of register
// 8s + j).  Weights: row-major bf16 images [out][in] per part in LDS with padded rows (odd
// multiples of 8 bytes: conflict-free row reads, linear addresses): the forward A fragments
// are two 8-byte row reads, the backward (W^T) ones two ds_read_b64_tr_b16 transposed reads
// of the same image.  Weight gradients sum over the tile's 32 rows: both operands go
// through one per-wave bf16 image [row][feature] of the split parts, read back transposed.
// In here: the split (split_pair .. split_step, split_l1 / split_l2), the six-product MFMA
// groups on VGPR (mfma6) and AGPR (macc6_16 .. macc_drain2, mac1) accumulators, with and without
// the next fragment's image reads in their gaps (macc6_rd: tools/check_asm_rd.py checks the built
// code), the weight- and tile-image reads and writes, the f32 transpose image's row sums, the
// hand-placed passes' placement plans (Plan, weave) and the packed parameter offsets (Packed).
// Part of the mlp_train.hip translation unit (one anonymous namespace); not for inclusion elsewhere.
#pragma once
#include "mlp_tile.h"

namespace {
namespace x3 {
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef short v4i16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4i16 lds_v4i16;

struct F3 {  // one MFMA operand fragment (8 elements) as its three bf16 parts
  u32x4 p[3];
};

// row strides (bytes) of the bf16 images: odd multiples of 8 B over the data width
constexpr int W2_ROWB = 72, W3_ROWB = 136, IM_ROWB = 72;
constexpr int W2_PART = 64 * W2_ROWB, W3_PART = 32 * W3_ROWB, IM_PART = 32 * IM_ROWB;
constexpr int IMG = 3 * IM_PART;    // one tile image (three parts) = the per-wave LDS slot
constexpr int TS = 36;              // f32 transpose image row stride (floats; 16-B aligned rows)
static_assert(32 * TS * 4 <= IMG, "the f32 image shares the slot");
constexpr int WAVES = 4;  // one wave per SIMD (512 registers)
// LDS image round trips within one wave: a wave's LDS instructions execute in issue order,
// so only the compiler must keep the write -> read order (no lgkmcnt drain)
__device__ __forceinline__ void lds_order() { asm volatile("" ::: "memory"); }

// x[l] + x[l ^ 32] (the two half-wave partial sums of a row) through v_permlane32_swap: no LDS
// round trip on the loss section's serial chain (ds_bpermute's latency).  The same bits as
// x + __shfl_xor(x, 32): lanes 32-63 add the same two values in the other order.
__device__ __forceinline__ float xhalf_sum(float x) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// the C-layout broadcast of a per-feature vector b (register r of lane half kh = b[feature]):
// a bias as an MFMA chain's initial accumulator, or w4 for the output layer
__device__ __forceinline__ f32x16 feat_vec(const float *b, int kh) {
  const float4 *b4 = reinterpret_cast<const float4 *>(b);
  f32x16 v;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const float4 c = b4[2 * q + kh];
    v[4 * q + 0] = c.x;
    v[4 * q + 1] = c.y;
    v[4 * q + 2] = c.z;
    v[4 * q + 3] = c.w;
  }
  return v;
}
// ReLU of an MFMA result as one integer max on the bits (signed compare orders non-negative
// floats like their values and sends every negative one, -0 included, to +0); fmaxf would
// first canonicalize the register (a second VALU op per element)
__device__ __forceinline__ float relu_bits(float x) { return __int_as_float(max(__float_as_int(x), 0)); }
__device__ __forceinline__ void relu16(f32x16 &v) {
#pragma unroll
  for (int r = 0; r < 16; r++) v[r] = relu_bits(v[r]);
}
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_bf16(float x, float y) {  // one v_cvt_pk_bf16_f32
  const f32x2 v = {x, y};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
// x - (the bf16 in the low / high half of h, as f32): the residual of a split level (exact: x and
// the bf16 rounding of x differ by a representable amount).  (One v_dot2c_f32_bf16 against
// (-1, 0) / (0, -1) instead of the back-conversion + subtraction pair: 1 437 instead of 1 560
// instructions per critic tile but +85 s_nop and +53 v_mov, train launch +6 %,
// profiles/r06_x3/ab_dot2_split.txt, tools/patches/x3_r06_dot2_split.patch.)
__device__ __forceinline__ float res_lo(uint32_t h, float x) { return x - __uint_as_float(h << 16); }
__device__ __forceinline__ float res_hi(uint32_t h, float y) { return y - __uint_as_float(h & 0xffff0000u); }
// (x, y) -> three packed bf16 pairs, x = hi + mid + lo exactly (element 0 in the low half)
__device__ __forceinline__ void split_pair(float x, float y, uint32_t &h, uint32_t &m, uint32_t &lo) {
  h = pk_bf16(x, y);
  const float x1 = res_lo(h, x), y1 = res_hi(h, y);
  m = pk_bf16(x1, y1);
  lo = pk_bf16(res_lo(m, x1), res_hi(m, y1));
}
// fragment element j = v[j]
__device__ __forceinline__ F3 split8(const float *v) {
  F3 f;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    uint32_t a, b, c;
    split_pair(v[2 * q], v[2 * q + 1], a, b, c);
    f.p[0][q] = a;
    f.p[1][q] = b;
    f.p[2][q] = c;
  }
  return f;
}
// K-step s of a C tile (registers 8s .. 8s+7) as a B (or A) fragment
__device__ __forceinline__ F3 split_step(const f32x16 &c, int s) {
  float v[8];
#pragma unroll
  for (int q = 0; q < 8; q++) v[q] = c[8 * s + q];
  return split8(v);
}

__device__ __forceinline__ f32x16 mfma_b(u32x4 a, u32x4 b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0,
                                                  0, 0);
}
// C += A B on split operands: the six products of combined order <= 2, smallest first
__device__ __forceinline__ f32x16 mfma6(const F3 &a, const F3 &b, f32x16 c) {
  c = mfma_b(a.p[2], b.p[0], c);
  c = mfma_b(a.p[0], b.p[2], c);
  c = mfma_b(a.p[1], b.p[1], c);
  c = mfma_b(a.p[1], b.p[0], c);
  c = mfma_b(a.p[0], b.p[1], c);
  return mfma_b(a.p[0], b.p[0], c);
}

// Weight-gradient accumulation C += A B (six products, as mfma6) with the accumulator pinned
// to AGPRs: it is touched by nothing but these MFMAs inside the loop, so it never moves
// between the register files and the arch VGPRs stay free for the tile's values.  Written as
// one asm block: "s_nop 1" covers the VALU-write -> MFMA-read hazard on A / B (the compiler
// cannot see the MFMAs inside), and back-to-back accumulation into the same AGPRs needs none.
#define X3_MACC6_BODY(OP)                                                                                \
  "s_nop 1\n\t" OP " %0, %3, %4, %0\n\t" OP " %0, %1, %6, %0\n\t" OP " %0, %2, %5, %0\n\t" OP " %0, %2, %4, %0\n\t" OP \
  " %0, %1, %5, %0\n\t" OP " %0, %1, %4, %0"                                                                      \
      : "+a"(c)                                                                                                      \
      : "v"(a.p[0]), "v"(a.p[1]), "v"(a.p[2]), "v"(b.p[0]), "v"(b.p[1]), "v"(b.p[2])
// (dW1's input columns past the first 16: a 16x16x32 block with no image reads in its gaps)
__device__ __forceinline__ void macc6_16(const F3 &a, const F3 &b, f32x4 &c) {
  asm(X3_MACC6_BODY("v_mfma_f32_16x16x32_bf16"));
}
// C += A B (six products, as macc6_16) with the next fragment's six transposed image reads issued
// in the MFMA gaps (an LDS read between two 32x32x16 MFMAs costs the wave almost nothing, a run
// of them costs their issue and puts their latency in front of the MFMAs that need them).  The
// compiler does not see these reads: WAIT puts an lgkmcnt(0) in front of a block whose B
// fragment came from the previous block's reads (LDS returns in order, so the compiler's own
// counted waits stay sufficient with them in flight).  nx <- image K-step rows at rbase + off.
#define X3_MACC6_RD(NAME, ACC, OP)                                                                          \
  template <bool WAIT, int OFF>                                                                              \
  __device__ __forceinline__ void NAME(const F3 &a, const F3 &b, ACC &c, F3 &nx, const char *rbase) {       \
    constexpr int U = 4 * IM_ROWB;                                                                           \
    const uint32_t ad = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char *)rbase;         \
    uint2 r0, r1, r2, r3, r4, r5;                                                                            \
    if constexpr (WAIT) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                  \
    asm volatile("s_nop 1\n\t" OP " %0, %9, %10, %0\n\tds_read_b64_tr_b16 %1, %13 offset:%14\n\t" OP          \
                 " %0, %7, %12, %0\n\tds_read_b64_tr_b16 %2, %13 offset:%15\n\t" OP                           \
                 " %0, %8, %11, %0\n\tds_read_b64_tr_b16 %3, %13 offset:%16\n\t" OP                           \
                 " %0, %8, %10, %0\n\tds_read_b64_tr_b16 %4, %13 offset:%17\n\t" OP                           \
                 " %0, %7, %11, %0\n\tds_read_b64_tr_b16 %5, %13 offset:%18\n\t" OP                           \
                 " %0, %7, %10, %0\n\tds_read_b64_tr_b16 %6, %13 offset:%19"                                 \
                 : "+a"(c), "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5)                 \
                 : "v"(a.p[0]), "v"(a.p[1]), "v"(a.p[2]), "v"(b.p[0]), "v"(b.p[1]), "v"(b.p[2]), "v"(ad),    \
                   "i"(OFF), "i"(OFF + U), "i"(OFF + IM_PART), "i"(OFF + IM_PART + U), "i"(OFF + 2 * IM_PART), \
                   "i"(OFF + 2 * IM_PART + U)                                                                \
                 : "memory");                                                                                \
    nx.p[0] = u32x4{r0.x, r0.y, r1.x, r1.y};                                                                  \
    nx.p[1] = u32x4{r2.x, r2.y, r3.x, r3.y};                                                                  \
    nx.p[2] = u32x4{r4.x, r4.y, r5.x, r5.y};                                                                  \
  }
X3_MACC6_RD(macc6_rd, f32x16, "v_mfma_f32_32x32x16_bf16")
X3_MACC6_RD(macc6_16_rd, f32x4, "v_mfma_f32_16x16x32_bf16")
#undef X3_MACC6_RD
// the last block of a chain: wait for its asm-read fragment, then the six MFMAs — ONE volatile
// statement: as two, the compiler may hoist the (non-volatile) MFMA block above the wait, and the
// MFMAs then read registers whose LDS data is still in flight (tools/check_asm_rd.py found
// exactly that in the actor's last dW3 block before this was one statement)
#define X3_MACC6_W(OP) asm volatile("s_waitcnt lgkmcnt(0)\n\t" X3_MACC6_BODY(OP) : "memory")
__device__ __forceinline__ void macc6_w(const F3 &a, const F3 &b, f32x16 &c) { X3_MACC6_W("v_mfma_f32_32x32x16_bf16"); }
__device__ __forceinline__ void macc6_16_w(const F3 &a, const F3 &b, f32x4 &c) { X3_MACC6_W("v_mfma_f32_16x16x32_bf16"); }
#undef X3_MACC6_W
#undef X3_MACC6_BODY
// C += A B for a B whose mid / lo parts are zero (the one-hot bias-sum columns: bf16 1.0 is exact),
// three products, smallest first, accumulator in AGPRs.  Volatile: its A may be a fragment an
// earlier asm block read, and it must stay behind the wait that completed it.
__device__ __forceinline__ void macc3(const F3 &a, const u32x4 &b, f32x16 &c) {
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %3, %4, %0\n\tv_mfma_f32_32x32x16_bf16 %0, %2, %4, %0\n\t"
               "v_mfma_f32_32x32x16_bf16 %0, %1, %4, %0"
               : "+a"(c)
               : "v"(a.p[0]), "v"(a.p[1]), "v"(a.p[2]), "v"(b));
}
// before the accumulators are read: the last MFMA's result latency (>= 18 passes)
__device__ __forceinline__ void macc_drain(f32x16 &a, f32x16 &b, f32x16 &c, f32x16 &d, f32x4 &e, f32x4 &f) {
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" : "+a"(a), "+a"(b), "+a"(c), "+a"(d), "+a"(e), "+a"(f));
}
__device__ __forceinline__ void macc_drain2(f32x16 &a, f32x16 &b, f32x16 &c, f32x16 &d, f32x4 &e, f32x4 &f,
                                            f32x4 &g, f32x4 &h) {
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" : "+a"(a), "+a"(b), "+a"(c), "+a"(d), "+a"(e), "+a"(f), "+a"(g),
               "+a"(h));
}
__device__ __forceinline__ uint2 lds_u2(const char *p) { return *reinterpret_cast<const uint2 *>(p); }
__device__ __forceinline__ uint2 tr16(const char *p) {
  v4i16 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4i16 *)(p));
  return __builtin_bit_cast(uint2, v);
}
// two 8-byte reads (at p and p + du) of each part -> fragment elements 0-3 / 4-7
template <int PART>
__device__ __forceinline__ F3 rd_pair(const char *p, int du) {
  F3 f;
#pragma unroll
  for (int pt = 0; pt < 3; pt++) {
    const uint2 a = lds_u2(p + pt * PART), b = lds_u2(p + pt * PART + du);
    f.p[pt] = u32x4{a.x, a.y, b.x, b.y};
  }
  return f;
}
template <int PART>
__device__ __forceinline__ F3 tr_pair(const char *p, int du) {
  F3 f;
#pragma unroll
  for (int pt = 0; pt < 3; pt++) {
    const uint2 a = tr16(p + pt * PART), b = tr16(p + pt * PART + du);
    f.p[pt] = u32x4{a.x, a.y, b.x, b.y};
  }
  return f;
}
// Lane address bases (loop invariants; every fragment is base + a compile-time offset):
//  row read   (forward A of W, lane row r, half h): r * ROWB + 8 h; K-step s, u -> + 8 (4s + 2u)
//  transposed (W^T A / image B, lane 16G + 4q + p): (4 (G>>1) + q) * ROWB... see below
// Forward A fragment of W (rows `out` = base row + 32 t), K-step s, permuted k order:
// element j <- in feature 16s + 8(j>>2) + 4h + (j&3), i.e. 8-byte chunk 4s + 2u + h.
template <int ROWB, int PART>
__device__ __forceinline__ F3 w_fwd(const char *rowbase, int t, int s) {
  return rd_pair<PART>(rowbase + t * 32 * ROWB + 32 * s, 16);
}
// Backward A fragment of W^T (lane: in feature 32t + (l & 31)), K-step s over the out
// features in the permuted order: element j <- W[16s + 8(j>>2) + 4h + (j&3)][in]; lane
// 4q + p of group G addresses row 16s + 8u + 4(G>>1) + q, chunk 8t + 4(G&1) + p
// (trbase = W + (4 (G>>1) + q) * ROWB + 8 (4 (G&1) + p)).
template <int ROWB, int PART>
__device__ __forceinline__ F3 w_bwd(const char *trbase, int t, int s) {
  return tr_pair<PART>(trbase + 16 * s * ROWB + 64 * t, 8 * ROWB);
}
// Tile image [32 rows][32 features] of a C tile given as its two split K-step fragments:
// lane (row r, half h) writes register group g (features 8g + 4h .. +3) as chunk 2g + h
// (wbase = img + r * IM_ROWB + 8 h).
template <int PART = IM_PART>
__device__ __forceinline__ void img_write(char *wbase, const F3 &f0, const F3 &f1) {
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const F3 &f = g < 2 ? f0 : f1;
    const int q = 2 * (g & 1);
#pragma unroll
    for (int pt = 0; pt < 3; pt++)
      *reinterpret_cast<uint2 *>(wbase + pt * PART + 16 * g) = make_uint2(f.p[pt][q], f.p[pt][q + 1]);
  }
}
// one half of one part (hi / mid / lo) of img_write: ONE 16-byte-per-lane LDS store (a
// ds_write2_b64), register groups 2 hf and 2 hf + 1 of part pt (f = f0 for hf 0, f1 for hf 1).  The
// hand-placed passes issue an image as six of these, at most one per two MFMA shadows: with four
// waves storing, a store after every MFMA costs each wave 27 cycles per store, two after every MFMA
// 95, one after every second MFMA nothing (MI355X_MICROARCH.md §LDS; tools/probes/lds_store_mfma.hip,
// profiles/r05_lds_store/)
__device__ __forceinline__ void img_write_h(char *wbase, const F3 &f, int pt, int hf) {
  *reinterpret_cast<uint2 *>(wbase + pt * IM_PART + 32 * hf) = make_uint2(f.p[pt][0], f.p[pt][1]);
  *reinterpret_cast<uint2 *>(wbase + pt * IM_PART + 32 * hf + 16) = make_uint2(f.p[pt][2], f.p[pt][3]);
}
// one part of a transposed fragment read (tr_pair): two ds_read_b64_tr_b16
__device__ __forceinline__ void tr_pt(const char *p, int du, int pt, F3 &f) {
  const uint2 a = tr16(p + pt * IM_PART), b = tr16(p + pt * IM_PART + du);
  f.p[pt] = u32x4{a.x, a.y, b.x, b.y};
}
// K-step s (rows 16s .. 16s+15) of the image read transposed: lane (feature l & 31, half h)
// gets rows 16s + 8h + j, j = 0..7; lane 4q + p of group G addresses row 16s + 8(G>>1) +
// 4u + q, chunk 4(G&1) + p (rbase = img + (8 (G>>1) + q) * IM_ROWB + 8 (4 (G&1) + p)).
__device__ __forceinline__ F3 img_read(const char *rbase, int s) {
  return tr_pair<IM_PART>(rbase + 16 * s * IM_ROWB, 4 * IM_ROWB);
}
// f32 transpose image T[feature][row] (stride TS) of a C tile, and the half-row sum of
// feature (l & 31) over rows 16h .. 16h+15 (the halves are combined once, at the end)
__device__ __forceinline__ void put_t(float *T, const f32x16 &v, int l) {
  float *b = T + 4 * (l >> 5) * TS + (l & 31);  // lane base; register r at a constant offset
#pragma unroll
  for (int r = 0; r < 16; r++) b[((r & 3) + 8 * (r >> 2)) * TS] = v[r];
}
#define X3_ROWSUM(k, v) \
  do {                   \
    put_t(T, v, l);      \
    lds_order();         \
    radd(k, half_row_sum(T, l)); \
    lds_order();         \
  } while (0)
__device__ __forceinline__ float half_row_sum(const float *T, int l) {
  const float4 *p = reinterpret_cast<const float4 *>(T + (l & 31) * TS + 16 * (l >> 5));
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const float4 v = p[c];
    s += v.x;
    s += v.y;
    s += v.z;
    s += v.w;
  }
  return s;
}
// stage one f32 weight element (split) into a row-major bf16 image
__device__ __forceinline__ void stage_w(char *Wimg, int part, int rowb, int row, int col, float w) {
  const __bf16 hi = (__bf16)w;
  const float r1 = w - (float)hi;
  const __bf16 mid = (__bf16)r1;
  const __bf16 lo = (__bf16)(r1 - (float)mid);
  const int off = row * rowb + col * 2;
  *reinterpret_cast<__bf16 *>(Wimg + off) = hi;
  *reinterpret_cast<__bf16 *>(Wimg + part + off) = mid;
  *reinterpret_cast<__bf16 *>(Wimg + 2 * part + off) = lo;
}
// d = (h > 0) ? d : 0 (ReLU derivative)
__device__ __forceinline__ void relu_mask(f32x16 &d, const f32x16 &h) {
#pragma unroll
  for (int r = 0; r < 16; r++) d[r] = h[r] > 0.0f ? d[r] : 0.0f;
}

// ---- Hand-placed passes (cfg::*::HAND_PLACED, mlp_x3.h): each block of MFMAs carries the NEXT
// block's VALU / LDS work in its MFMA shadows.  One wave per SIMD issues in order: a run of back-to-back MFMAs leaves
// the vector issue idle for 24 of every 32 cycles, a run of VALU leaves the matrix pipe idle, and
// the compiler cannot place VALU between the MFMAs of an opaque inline-asm block.  So every MFMA
// is its own statement and `weave` cuts the block into regions (sched_barrier: nothing crosses),
// region k = MFMA k + a share of the payload units, spread evenly (unit u in region u NMU / NU).
template <int B, int E, class F>
__device__ __forceinline__ void sfor(F &&f) {
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    sfor<B + 1, E>(f);
  }
}
// A payload plan: segments {first region, end region, units}, the units numbered in segment order
// and spread evenly over their segment's regions (unit t of a segment in r0 + t (r1 - r0) / n).
template <int... S>
struct Plan {
  static constexpr int NS = sizeof...(S) / 3;
  static constexpr int s[sizeof...(S)] = {S...};
  static constexpr int units() {
    int n = 0;
    for (int i = 0; i < NS; i++) n += s[3 * i + 2];
    return n;
  }
  static constexpr int NU = units();
  static constexpr int reg(int u) {  // the region of unit u
    for (int i = 0; i < NS; i++) {
      const int n = s[3 * i + 2];
      if (u < n) return s[3 * i] + u * (s[3 * i + 1] - s[3 * i]) / n;
      u -= n;
    }
    return -1;
  }
  static constexpr int first(int seg) {  // the first unit of segment seg
    int n = 0;
    for (int i = 0; i < seg; i++) n += s[3 * i + 2];
    return n;
  }
  static_assert(sizeof...(S) % 3 == 0, "plan: {r0, r1, units} triples");
};
// region k = MFMA k (mf(k)), then the payload units the plan puts in region k; nothing crosses a
// region border (sched_barrier)
template <int NM, class PL, class M, class U>
__device__ __forceinline__ void weave(M &&mf, U &&un) {
  static_assert(PL::NU == 0 || PL::reg(PL::NU - 1) < NM, "plan: units past the block's last region");
  sfor<0, NM>([&](auto kc) {
    constexpr int K = decltype(kc)::value;
    mf(kc);
    sfor<0, PL::NU>([&](auto uc) {
      if constexpr (PL::reg(decltype(uc)::value) == K) un(uc);
    });
    __builtin_amdgcn_sched_barrier(0);
  });
}
// the six products of a split x split MFMA (mfma6 order, smallest first) and the three of a
// split x one-hot one (macc3)
constexpr int P6A[6] = {2, 0, 1, 1, 0, 0}, P6B[6] = {0, 2, 1, 0, 1, 0};
// one weight-gradient MFMA, accumulator in AGPRs (volatile: kept in its region).  Its A / B come
// from LDS reads (or loop-invariant registers), never from a VALU write just before it: no wait
// states needed (tools/check_asm_rd.py checks the built code)
__device__ __forceinline__ void mac1(const u32x4 &a, const u32x4 &b, f32x16 &c) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
// the bias-sum MFMA: B = a loop-invariant one-hot fragment, kept in AGPRs (an MFMA reads A / B from
// either file; as "v" the compiler would copy it from the AGPR it parks it in right before the MFMA,
// a VALU write the MFMA then reads without its two wait states)
__device__ __forceinline__ void mac1_oh(const u32x4 &a, const u32x4 &oh, f32x16 &c) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "a"(oh));
}
__device__ __forceinline__ void mac1_16(const u32x4 &a, const u32x4 &b, f32x4 &c) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}
// The regions hold because no scheduler moves an instruction across a region barrier
// (sched_barrier(0)).  (Pinning the units with empty volatile asm statements instead cost one copy
// and one wait state per pinned value.)
// opaque loaded values: unconditional loads (hipcc otherwise turns `cond ? load : const` into a
// branch around the load); all of a unit's loads are pinned in ONE statement, after the last one
// is issued, so they wait once, together
__device__ __forceinline__ void pin4(float *v) { asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3])); }
// split level 1 of element pair q of an 8-element fragment v: hi part, residuals r[2q], r[2q+1]
__device__ __forceinline__ void split_l1(const float *v, int q, F3 &f, float *r) {
  const uint32_t h = pk_bf16(v[2 * q], v[2 * q + 1]);
  f.p[0][q] = h;
  r[2 * q] = res_lo(h, v[2 * q]);
  r[2 * q + 1] = res_hi(h, v[2 * q + 1]);
}
// split levels 2-3 of pair q from its residuals (as split_pair: the same bits)
__device__ __forceinline__ void split_l2(int q, F3 &f, const float *r) {
  const uint32_t m = pk_bf16(r[2 * q], r[2 * q + 1]);
  f.p[1][q] = m;
  f.p[2][q] = pk_bf16(res_lo(m, r[2 * q]), res_hi(m, r[2 * q + 1]));
}
// ReLU-derivative mask of elements r, r + 1 of d by h > 0
__device__ __forceinline__ void mask2(f32x16 &d, const f32x16 &h, int r) {
  d[r] = h[r] > 0.0f ? d[r] : 0.0f;
  d[r + 1] = h[r + 1] > 0.0f ? d[r + 1] : 0.0f;
}
__device__ __forceinline__ void relu4(f32x16 &h, int r0) {
#pragma unroll
  for (int r = r0; r < r0 + 4; r++) h[r] = relu_bits(h[r]);
}

// packed torch-layout offsets of one Model_PPO (W1 b1 W2 b2 W3 b3 W4 b4)
struct Packed {
  int W1, B1, W2, B2, W3, B3, W4, B4, NP;
  __host__ __device__ constexpr Packed(int nin, int nout)
      : W1(0), B1(32 * nin), W2(B1 + 32), B2(W2 + 64 * 32), W3(B2 + 64), B3(W3 + 32 * 64), W4(B3 + 32),
        B4(W4 + 32 * nout), NP(B4 + nout) {}
};
}  // namespace x3
}  // namespace
