// mlp_tile.h — what both train-kernel families (mlp_train_f32.h, mlp_x3.h) share: the head kinds
// and packed-parameter sizes, the f32 kernel's LDS layout `Lay` (the split kernel's 13-input
// geometry reuses its input-slot layout and its loaders), wave-level helpers (wave_sync, SGPR
// pinning), raw-buffer / LDS-DMA access with the hand-counted vmcnt wait, and the loaders of one
// 32-row tile's inputs into a wave's LDS slot: by LDS-DMA one tile ahead (prefetch_tile) or
// through registers (load_tile_regs / store_tile_regs, load_tile_sync for a ragged last tile).
// An input slot is X [32][n_in] | s0 = [ret | V] | s1 = [act | logp_old]; rows past the batch
// read as zeros (buffer range checks), never as memory outside the buffers.
// Part of the mlp_train.hip translation unit (one anonymous namespace); not for inclusion elsewhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

namespace {
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { K_CRITIC = 0, K_CONT = 1, K_CHOICE = 2 };  // the loss a head is trained on (mlp_train_f32.h)
constexpr int NIN_CONT = 13;
constexpr int S2 = 33, S3 = 65, ST = 33;  // LDS row strides (W2, W3, transpose tiles)
constexpr int TILE = 32 * ST;             // one transposed 32x32 tile

__host__ __device__ constexpr int n_params(int nin, int nout) {
  return 32 * nin + 32 + 64 * 32 + 64 + 32 * 64 + 32 + nout * 32 + nout;
}
constexpr int NIN_MAX = 64;  // choice heads: dc = 2 + 6(S-1) + 10 = 54 for the scalable 8-slot env
constexpr int NW_MAX = n_params(NIN_MAX, 2);

// LDS layout (floats) of one instantiation: KS = layer-1 k-steps (inputs padded to 2 KS),
// PF = double-buffered DMA prefetch (13-input heads), NOUT = output width.
template <int KS, bool PF, int NOUT>
struct Lay {
  static constexpr int WAVES = PF ? 8 : 4;  // PF: 2 waves/SIMD (<= 256 VGPRs); else 1
  static constexpr int S1 = 2 * KS + 1;     // odd W1 row stride
  static constexpr int O_W1 = 0, O_B1 = 32 * S1, O_W2 = O_B1 + 32, O_B2 = O_W2 + 64 * S2, O_W3 = O_B2 + 64,
                       O_B3 = O_W3 + 32 * S3, O_W4 = O_B3 + 32, O_B4 = O_W4 + 32 * NOUT,
                       O_WEND = (O_B4 + NOUT + 3) / 4 * 4;
  // per-wave input slot: X [32][n_in], s0 = [ret 32 | V 32], s1 = [act or logp_old 32 | logp_old 32]
  static constexpr int XMAX = PF ? 32 * NIN_CONT : 64 * KS;
  // PF: 32 floats of pad after s1 take the unpredicated DMAs' overhang (prefetch_tile)
  static constexpr int IN_X = 0, IN_S0 = XMAX, IN_S1 = IN_S0 + 64, IN_SZ = IN_S1 + 64 + (PF ? 32 : 0);
  static constexpr int NSLOT = PF ? 2 : 1;
  // per-wave scratch: 3 transpose tiles, then the input slot(s)
  static constexpr int O_T = 0, O_IN = 3 * TILE, WAVE_LDS = O_IN + NSLOT * IN_SZ;
  static constexpr int O_DACC = O_WEND + WAVES * WAVE_LDS;  // float64 [WAVES][3][32]
  static constexpr int FLOATS = O_DACC + WAVES * 3 * 32 * 2;
  static_assert(FLOATS * 4 <= 160 * 1024, "LDS budget");
  static_assert(O_WEND % 4 == 0 && WAVE_LDS % 4 == 0 && O_IN % 4 == 0 && IN_SZ % 4 == 0, "16-B aligned slots");
};

// the feature held by C register r of lane l (the orientation note in mlp_train_f32.h)
__device__ __forceinline__ int feat(int r, int l) { return (r & 3) + 8 * (r >> 2) + 4 * (l >> 5); }
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// wave-uniform values pinned to SGPRs (the compiler otherwise holds some in VGPRs)
__device__ __forceinline__ float uniform_f(float x) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
__device__ __forceinline__ int64_t uniform_i64(int64_t x) {
  const uint64_t u = (uint64_t)x;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ double uniform_d(double x) {
  return __longlong_as_double(uniform_i64(__double_as_longlong(x)));
}
__device__ __forceinline__ f32x16 zero16() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; i++) z[i] = 0.0f;
  return z;
}

// Raw buffer resource over [p, p + bytes): SGPR base, 32-bit VGPR lane offsets (no 64-bit
// per-lane pointers for the compiler to hoist and spill), hardware range check (loads past
// `bytes` return 0, stores past it are dropped).  dword3 = gfx9 raw-buffer format.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}
// LDS-DMA (buffer_load ... lds): lane l's dword(s) land at lds_base + l * size, lds_base
// wave-uniform (M0).  Issued from inline asm so the compiler's waitcnt pass does not see
// it: the pass cannot tell the DMA'd slot from other LDS and would put vmcnt(0) before
// every LDS read, draining the prefetch; the kernel counts vmcnt itself (wait_vmcnt).
typedef int v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4i rsrc_v(const void *p, uint32_t bytes) {
  const uint64_t a = (uint64_t)p;
  v4i d;
  d.x = (int)(uint32_t)a;
  d.y = (int)(uint32_t)(a >> 32) & 0xffff;  // stride 0
  d.z = (int)bytes;
  d.w = 0x00020000;
  return d;
}
__device__ __forceinline__ uint32_t lds_addr(const float *p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float *)p;
}
__device__ __forceinline__ void dma16(v4i r, const float *lds_base, uint32_t voff) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(r), "s"(lds_addr(lds_base))
      : "memory");
}
__device__ __forceinline__ void dma4(v4i r, const float *lds_base, uint32_t voff) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dword %1, %2, 0 offen lds\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(r), "s"(lds_addr(lds_base))
      : "memory");
}
__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, uint32_t voff) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, 0, 0));
}
// s_waitcnt vmcnt(N) (gfx9 encoding: vmcnt[3:0], expcnt[6:4] = 7, lgkmcnt[11:8] = 15)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N < 16, "vmcnt");
  __builtin_amdgcn_s_waitcnt(0x0F70 | N);
}

// Inputs of one full 32-row tile -> an input slot, by LDS-DMA (no VGPRs, no wait here).
// X: 416 contiguous floats = 104 16-B chunks (64 + 40 lanes); s0/s1: one dword per lane,
// exec masks pick the lanes (a DMA's inactive lanes write nothing).
// Every DMA's buffer range is bounded by the rows the batch really has past row0 (M): a tile index
// past the batch (a prefetch-ring or tile-loop indexing error) reads zeros instead of touching
// memory outside the buffers (the raw-buffer range check bounds the offset from the base; with a
// zero range nothing is fetched, whatever the base).  Full tiles: the same 32-row ranges.
__device__ __forceinline__ uint32_t tile_rows(int64_t M, int64_t row0) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)max((int64_t)0, min((int64_t)32, M - row0)));
}
template <int KIND, class LY>
__device__ __forceinline__ void prefetch_tile(float *slot, const float *X, const float *ret, const float *V,
                                              const float *act, const float *lp, int64_t row0, int l, int64_t M) {
  const uint32_t rows = tile_rows(M, row0);
  const v4i rx = rsrc_v(X + row0 * NIN_CONT, rows * NIN_CONT * 4);
  // Every DMA on all 64 lanes (no exec-mask branches): an LDS-DMA lane writes base + 4 lane, so
  // the lanes past a piece's end land in the NEXT piece's place (or the 32-float pad after s1),
  // reading zeros past their buffer's bounds; the pieces are issued in address order and their
  // LDS writes land in issue order, so each overhang is overwritten by the piece it covers.
  dma16(rx, slot + LY::IN_X, 16 * l);
  dma16(rx, slot + LY::IN_X + 256, 1024 + 16 * l);  // X 256..415; lanes 40-63: zeros into s0
  const uint32_t vo = 4 * l;
  dma4(rsrc_v(ret + row0, 4 * rows), slot + LY::IN_S0, vo);  // ret [0, 32); lanes 32-63: zeros [32, 64)
  if (KIND == K_CONT) {
    dma4(rsrc_v(V + row0, 4 * rows), slot + LY::IN_S0 + 32, vo);   // V [32, 64); overhang into s1
    dma4(rsrc_v(act + row0, 4 * rows), slot + LY::IN_S1, vo);      // act [0, 32); overhang [32, 64)
    dma4(rsrc_v(lp + row0, 4 * rows), slot + LY::IN_S1 + 32, vo);  // logp_old [32, 64); overhang: pad
  }
}
template <int KIND>
constexpr int prefetch_ops() { return KIND == K_CRITIC ? 3 : 6; }  // DMA instructions per prefetch

// Tile inputs through registers: load_tile_regs issues every load of a 32-row tile (X rows,
// the s0/s1 targets) with none waiting on another; store_tile_regs writes them to the wave's
// input slot.  A runtime-trip-count load -> store loop would wait one memory round trip per 64
// floats (15 per tile at n_in = 30).  Rows past M read as 0 (buffer bounds).
template <class LY>
struct TileRegs {
  float x[(LY::XMAX + 63) / 64];
  float s0, s1;
};
template <int KIND, class LY>
__device__ __forceinline__ void load_tile_regs(TileRegs<LY> &t, const float *X, int nin, const float *ret,
                                               const float *V, const float *act, const float *lp, int64_t row0,
                                               int nrows, int l) {
  const auto rx = rsrc(X + row0 * nin, (uint32_t)(nrows * nin) * 4);
#pragma unroll
  for (int i = 0; i < (LY::XMAX + 63) / 64; i++) {
    const int q = l + 64 * i;
    t.x[i] = q < 32 * nin ? bload(rx, 4 * q) : 0.0f;
  }
  const uint32_t nb = 4 * nrows, vo = 4 * (l & 31);
  t.s0 = bload(rsrc((l < 32 || KIND == K_CRITIC) ? ret + row0 : V + row0, nb), vo);
  t.s1 = 0.0f;
  if (KIND == K_CONT) t.s1 = bload(rsrc(l < 32 ? act + row0 : lp + row0, nb), vo);
  if (KIND == K_CHOICE)  // [logp_old 32 | action 32] (the action is read only in per-row mode)
    t.s1 = bload(rsrc((l < 32 || act == nullptr) ? lp + row0 : act + row0, nb), vo);
}
template <int KIND, class LY>
__device__ __forceinline__ void store_tile_regs(float *slot, const TileRegs<LY> &t, int nin, int l) {
#pragma unroll
  for (int i = 0; i < (LY::XMAX + 63) / 64; i++) {
    const int q = l + 64 * i;
    if (q < 32 * nin) slot[LY::IN_X + q] = t.x[i];
  }
  slot[LY::IN_S0 + l] = t.s0;
  if (KIND == K_CONT || KIND == K_CHOICE) slot[LY::IN_S1 + l] = t.s1;
}
// Synchronous tile load (ragged last tile of the DMA path)
template <int KIND, class LY>
__device__ __forceinline__ void load_tile_sync(float *slot, const float *X, int nin, const float *ret,
                                               const float *V, const float *act, const float *lp, int64_t row0,
                                               int nrows, int l) {
  TileRegs<LY> t;
  load_tile_regs<KIND, LY>(t, X, nin, ret, V, act, lp, row0, nrows, l);
  store_tile_regs<KIND, LY>(slot, t, nin, l);
}
}  // namespace
