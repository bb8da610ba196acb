// mlp_x3.h — the split-precision (bf16x3) train kernels k_mlp_train_x3<KIND, Geo> and
// k_mlp_train_x3_pair: the default train pass of every head with up to 54 inputs (the 13-input
// critic / continuous actor on the big batches, the choice heads' two nets).  The same fused
// forward + loss gradient + backward + weight gradient as the exact-f32 kernel
// (mlp_train_f32.h: the kinds, the orientation and the feature order are described there), with
// every GEMM on bf16 MFMA over exactly split operands (mlp_x3_prims.h).
// A block is 4 waves, one per SIMD (512 registers each: the weight-gradient accumulators and the
// loop-invariant weight fragments sit in AGPRs), and the grid is one block per CU, the waves
// grid-striding over 32-row tiles with the next tile's inputs landing by LDS-DMA in a
// double-buffered slot.  After its tile loop each wave writes its packed gradient to LDS, the block
// folds the four in fixed order to ONE float64 partial (fold_partials), and a single
// k_grad_reduce_blocks launch (mlp_grad_reduce.h) sums the block partials: deterministic.
// Measured alternatives to one wave per SIMD: two waves per SIMD at 256 registers
// (no hoisted fragments, h1 recomputed: 12 % slower), two tiles per wave in lock step (spills), a
// software-pipelined loop (backward of tile i beside the forward of tile i+1: 10 % slower).
// What a pass holds in registers and how its backward is placed is a named configuration
// (namespace cfg below), one per shipped pass.
//
// The continuous actor's ratio: its magnitude r = expf(lp - logp_old) in float32, its clip branch
// decided on the float64 difference lp - logp_old (surr_and_grad_fd: the decision of the
// reference's float64 ratio, Coop-MH-PPO-scalable.py:803-806), not a float64 exp.  The float64
// exp's temporaries kept W3's forward fragments out of the actor's registers (cfg::Actor13 fits at
// 510 VGPRs without them): cfg3 iteration -1.4 % over three interleaved bench pairs
// (profiles/r05_floss/); the float64-exp build on r06 driver-length benches: +1.1 % per iteration
// and the same gradient to 3 digits at bench scale with 23 % of the rows clipped
// (profiles/r06_a/).  Numerics: lp - logp_old in float32 is exact only while the two are within a
// factor 2 of each other (Sterbenz), which updates do not guarantee row by row, so r carries up to
// two float32 roundings (~1.2e-7 relative) — the level of the difference mu itself has from the
// reference's CPU GEMM; the clip decision carries none.  dmu's product stays
// float64 with one rounding: a float32 chain of four roundings there moved the 2-rank vs 1-rank
// nets of tests/test_dp_gpu.py from <= 7.6e-7 to 6.4e-5 (tools/dp_diff.py).  The exact f32
// kernel keeps the float64 ratio.
// Part of the mlp_train.hip translation unit (one anonymous namespace); not for inclusion elsewhere.
#pragma once
#include <math.h>

#include <type_traits>

#include "mlp_tile.h"
#include "mlp_x3_prims.h"
#include "ppo_heads.h"    // the heads' per-row arithmetic; surr_and_grad, surr_and_grad_fd (ppo_math.h)
#include "rollout_dev.h"  // MHPPO_MARK

using namespace mhppo;

namespace {
namespace x3 {
// Geometry of one split-precision net: K1 = layer-1 K (the inputs and the bias column, padded to
// whole 16-deep K-steps), NOUT outputs, NIC the compile-time input count (0: a kernel argument,
// nin <= NMX, by default K1 - 1).  LDS: the net's weights (bf16 images of W1..W3, f32 b2 b3 w4
// b4), then per wave: the tile image (also the f32 transpose image), two input slots (double
// buffered), a second tile image.
template <int K1_, int NOUT_, int NIC_, int NIM_ = 2, int NMX_ = K1_ - 1>
struct Geo {
  static constexpr int K1 = K1_, KS1 = K1 / 16, NOUT = NOUT_, NIC = NIC_, NIM = NIM_, NMX = NMX_;
  static_assert(K1 % 16 == 0 && (NIC == 0 || NIC < K1) && NMX < K1, "layer-1 geometry");
  static constexpr int W1_ROWB = 2 * K1 + 8, W1_PART = 32 * W1_ROWB;
  static constexpr int O_W1 = 0, O_W2 = O_W1 + 3 * W1_PART, O_W3 = O_W2 + 3 * W2_PART, O_F = O_W3 + 3 * W3_PART;
  static constexpr int F_W4 = 96, F_B4 = F_W4 + 32 * NOUT, NF = F_B4 + NOUT;  // f32: b2[64] b3[32] w4 b4
  static constexpr int NET_B = (O_F + NF * 4 + 15) / 16 * 16;
  // input slot (floats): X [32][nin] | s0 [32 | 32] | s1 [32 | 32].  A runtime nin gets an X region
  // of whole 1-KiB pieces, so every LDS-DMA piece lands unmasked (zeros past the rows).
  static constexpr int XMAX = NIC == NIN_CONT ? (32 * NIC + 3) / 4 * 4 : (32 * (NIC ? NIC : NMX) + 255) / 256 * 256;
  static constexpr int IN_X = 0, IN_S0 = XMAX, IN_S1 = XMAX + 64, IN_SZ = XMAX + 128 + (NIC ? 32 : 0);
  static constexpr int XPIECES = (XMAX * 4 + 1023) / 1024;
  // NIM tile-image slots per wave: slot 1 at 0, slot 2 at O_IM2, slots 3 and 4 after it (the
  // hand-placed passes write the forward's h1 / h2a images during the forward, into slots of their own)
  static constexpr int IMGA = (IMG + 15) / 16 * 16;
  static constexpr int O_IN = IMGA, O_IM2 = O_IN + 2 * IN_SZ * 4, O_IM3 = O_IM2 + IMGA, O_IM4 = O_IM3 + IMGA,
                       WAVE_B = O_IM2 + (NIM - 1) * IMGA;
  static constexpr int LDS_BYTES = NET_B + WAVES * WAVE_B;
  static constexpr int LDS_BYTES_PAIR = 2 * NET_B + WAVES * WAVE_B;  // two nets' weights (pair kernel)
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
  static_assert(WAVE_B % 16 == 0 && O_IN % 16 == 0 && IN_SZ % 4 == 0, "16-B aligned slots");
};
// the 13-input continuous heads (the big batches): the slot layout of the f32 path's Lay<7, true, 1>
using G13 = Geo<16, 1, NIN_CONT>;
using G13S = Geo<16, 1, NIN_CONT, 4>;  // the hand-placed single-net passes (four image slots per wave)
using LY = Lay<7, true, 1>;
static_assert(G13::IN_S0 == LY::IN_S0 && G13::IN_S1 == LY::IN_S1 && G13::IN_SZ == LY::IN_SZ, "13-input slot");
static_assert(G13::LDS_BYTES_PAIR <= 160 * 1024, "LDS budget (pair)");
// the choice heads' nets on this kernel: up to NIN_X3C inputs (wider ones stay on the f32 kernel).
// K = 64 (the scalable 8-slot env's dc = 54, Coop-MH-PPO-scalable.py:818-851): the input slots sized
// for 54 inputs (7 KiB of X rows), the four waves' slots and the weights then fit the 160 KiB of LDS
constexpr int NIN_X3C = 54;
using GC16 = Geo<16, 2, 0>;
using GV16 = Geo<16, 1, 0>;
using GC32 = Geo<32, 2, 0>;
using GV32 = Geo<32, 1, 0>;
using GC64 = Geo<64, 2, 0, 2, NIN_X3C>;
using GV64 = Geo<64, 1, 0, 2, NIN_X3C>;
// dc = 54 itself with a compile-time input count: the runtime count's address arithmetic spilled
// the choice actor (15 VGPRs at 512); compile-time: 496 VGPRs, no spill
using GC54 = Geo<64, 2, 54, 2, 54>;
using GV54 = Geo<64, 1, 54, 2, 54>;
template <class G>
__device__ __forceinline__ int geo_nin(int nin_rt) { return G::NIC ? G::NIC : nin_rt; }

// Stage one net's weights at Lw: bf16 images (three parts), b1 as input column nin of W1.  Every
// global load is issued before the first LDS store (one memory round trip per launch; a strided
// load -> split -> store loop per array costs one dependent trip per iteration).
template <class G>
__device__ __forceinline__ void stage_net(const float *__restrict__ W, char *Lw, int tid, int nin_rt) {
  const int nin = geo_nin<G>(nin_rt);
  const Packed P(nin, G::NOUT);
  constexpr int K1 = G::K1, NF = G::NF;
  float *F = reinterpret_cast<float *>(Lw + G::O_F);  // b2 [0, 64) b3 [64, 96) w4 [96, ...) b4
  constexpr int NT = 64 * WAVES, N1 = (32 * K1 + NT - 1) / NT, N2 = 2048 / NT, NFQ = (NF + NT - 1) / NT;
  static_assert(2048 % NT == 0, "staging: block size");
  float v1[N1], v2[N2], v3[N2], vf[NFQ];
#pragma unroll
  for (int q = 0; q < N1; q++) {
    const int i = tid + q * NT, r = i / K1, c = i % K1;
    v1[q] = i >= 32 * K1 ? 0.0f : (c < nin ? W[P.W1 + r * nin + c] : (c == nin ? W[P.B1 + r] : 0.0f));
  }
#pragma unroll
  for (int q = 0; q < N2; q++) {
    v2[q] = W[P.W2 + tid + q * NT];
    v3[q] = W[P.W3 + tid + q * NT];
  }
#pragma unroll
  for (int q = 0; q < NFQ; q++) {
    const int i = tid + q * NT;
    vf[q] = i < 64 ? W[P.B2 + i]
                   : (i < 96 ? W[P.B3 + i - 64]
                             : (i < G::F_B4 ? W[P.W4 + i - 96] : (i < NF ? W[P.B4 + i - G::F_B4] : 0.f)));
  }
#pragma unroll
  for (int q = 0; q < N1; q++) {
    const int i = tid + q * NT;
    if (i < 32 * K1) stage_w(Lw + G::O_W1, G::W1_PART, G::W1_ROWB, i / K1, i % K1, v1[q]);
  }
#pragma unroll
  for (int q = 0; q < N2; q++) {
    const int i = tid + q * NT;
    stage_w(Lw + G::O_W2, W2_PART, W2_ROWB, i >> 5, i & 31, v2[q]);
    stage_w(Lw + G::O_W3, W3_PART, W3_ROWB, i >> 6, i & 63, v3[q]);
  }
#pragma unroll
  for (int q = 0; q < NFQ; q++) {
    const int i = tid + q * NT;
    if (i < NF) F[i] = vf[q];
  }
}

// The per-wave lane geometry of the wave's LDS slot (images, f32 transpose image, input slots)
template <class GEO>
struct WaveSlot {
  char *wb;          // this wave's image / f32 transpose slot
  float *T;          // f32 transpose image (shares the slot)
  float *inb;        // input slots (double buffered)
  char *imw;         // image write base
  const char *imr;   // image transposed-read base (32x32x16 operands)
  const char *imr16; // image transposed-read base (16x16x32 operands)
  int l, j, kh, G;
  __device__ __forceinline__ WaveSlot(char *L8, int w, int l_) : l(l_), j(l_ & 31), kh(l_ >> 5), G(l_ >> 4) {
    const int q4 = (l >> 2) & 3, p4 = l & 3;
    wb = L8 + w * GEO::WAVE_B;
    T = reinterpret_cast<float *>(wb);
    inb = reinterpret_cast<float *>(wb + GEO::O_IN);
    imw = wb + j * IM_ROWB + 8 * kh;
    // image reads: rows 8 (G >> 1) + 4u + q, chunk 4 (G & 1) + p
    imr = wb + (8 * (G >> 1) + q4) * IM_ROWB + 8 * (4 * (G & 1) + p4);
    imr16 = wb + (8 * G + q4) * IM_ROWB + 8 * p4;  // 16x16x32 A: rows 8G + 4u + q, chunk 4t + p
  }
};

// What a pass keeps in registers across its tiles and how its backward is placed: one type per
// shipped pass (k_mlp_train_x3 picks it from (KIND, G) in pass_cfg; the pair kernel names its own).
//   HAND_PLACED  forward and backward placed by hand (layer1_s / fwd_s / bwd_s: every MFMA block
//                carries the next block's VALU / LDS work in its shadows), with W2's and W3's
//                forward fragments held in registers.  Only the 13-input single-net passes: the
//                phase-by-phase dW2 block needs those registers for the image reads it issues in
//                its MFMA gaps, and a second net in the same wave needs them too.
//   HOLD_BWD     the backward (W3^T, W2^T) fragments held in registers (not with two nets in a wave)
//   DW4_REGS     dW4 = sum over rows of dy h3 accumulated per lane and register across the wave's
//                tiles (one FMA per element) and summed over the lanes once, in finish, instead of a
//                per-tile LDS transpose (probe: -2.7 % actor tile time without that sum)
//   DH2_FIRST    phase-by-phase backward only: the on-chain dH2 MFMAs issued before the off-chain dW3
//                block (the h2 image splits in their shadow)
// Every pass sums dB3 / dB2 on the MFMA (Pass::gBS).
namespace cfg {
// The 13-input critic alone: 509 VGPRs, no spill.  The hand-placed forward writes the h images, which
// frees the registers for the forward fragments: W2's -2.1 %, W3's too a further -3.5 %
// (profiles/r05_x3/ab.txt, ab_hf3.txt).
struct Critic13 {
  static constexpr bool HAND_PLACED = true, HOLD_BWD = true, DW4_REGS = true, DH2_FIRST = false;
};
// The continuous actor alone: 510 VGPRs, no spill.  W2's forward fragments -1.5 % (485 VGPRs,
// profiles/r05_x3/ab.txt); W3's fit only with the float32 loss math (with a float64 exp they
// spilled 60 B; the note on the actor's ratio above).
struct Actor13 {
  static constexpr bool HAND_PLACED = true, HOLD_BWD = true, DW4_REGS = true, DH2_FIRST = false;
};
// The continuous actor and the critic of the fused pair kernel: two nets in one wave, so neither
// holds fragments.  dH2 first: -1.6 % (profiles/r04_x3_bs/ab_order.txt).  dW4 in registers for the
// critic too, as in its single pass: the same bits.
struct Pair13 {
  static constexpr bool HAND_PLACED = false, HOLD_BWD = false, DW4_REGS = true, DH2_FIRST = true;
};
// The choice head's critic (runtime or 54 inputs): forward fragments would spill 23-38 VGPRs, dH2
// first costs +3 % at its 512 registers; the launch floor dominates at its batch sizes
// (profiles/r04_x3_bs/README.md).
struct ChoiceCritic {
  static constexpr bool HAND_PLACED = false, HOLD_BWD = true, DW4_REGS = false, DH2_FIRST = false;
};
// The choice actor: as its critic; dW4 in registers for its second output would spill the K = 32
// geometry.
struct ChoiceActor {
  static constexpr bool HAND_PLACED = false, HOLD_BWD = true, DW4_REGS = false, DH2_FIRST = false;
};
}  // namespace cfg

// One net's pass over 32-row tiles (forward, loss gradient, backward, weight gradients), with its
// per-wave state: lane bases into its staged weights, the loop-invariant weight fragments, the
// weight-gradient accumulators and the bias / loss sums.
// G: the net's geometry (inputs, outputs); K_CHOICE: the choice actor (two outputs, softmax pair);
// CFG: one of the configurations above.
template <int KIND, class G, class CFG>
struct Pass {
  static constexpr int KS1 = G::KS1, NOUT = G::NOUT;
  static constexpr bool HAND_PLACED = CFG::HAND_PLACED, HOLD_BWD = CFG::HOLD_BWD, DW4_REGS = CFG::DW4_REGS;
  static_assert(!HAND_PLACED || (KS1 == 1 && HOLD_BWD && DW4_REGS && G::NIC == NIN_CONT && G::NIM == 4),
                "hand-placed: the 13-input single-net passes, four image slots");
  static_assert(!DW4_REGS || NOUT == 1, "dW4 in registers: one output (a second one's would spill)");
  static_assert(NOUT == (KIND == K_CHOICE ? 2 : 1), "outputs");
  const char *w1row, *w2row, *w3row, *w2tr, *w3tr;
  const float *F;
  float b40, b41;
  int nin;
  const double *counts;  // K_CHOICE: the global action counts (nullptr: per-row mode)
  double m_global;
  F3 wf2[2][2], wf3[4], wb3[2][2], wb2[4];
  // hand-placed: the previous tile's dW1 block (E), deferred into this tile's layer-1 shadows: its A operands
  // (the d1 image's transposed reads) and B operand (the input columns); zero before the first tile
  F3 ea0, ea1, exb;
  f32x16 gW2a, gW2b, gW3a, gW3b;
  f32x4 gW1t[KS1][2];
  // The bias gradients dB3 / dB2 as MFMA row sums of the d3 / d2 image fragments the weight
  // gradients already read (a one-hot B column each, three products) instead of a per-tile LDS
  // transpose and VALU sum each (probe: -5.6 % critic / -8.4 % actor tile time without those sums,
  // profiles/r04_x3_bs/): column 0 = dB3, 1 = dB2[0:32], 2 = dB2[32:64] (rows = out features)
  f32x16 gBS;
  u32x4 oh[3];  // B fragments with bf16 1.0 in column q only
  f32x16 gW4r;  // DW4_REGS: dW4 per lane and register (row j, features feat(r, l))
  // half-row sums (lane j, half kh): gW4[0] gB4[0] gW4[1] gB4[1] (gW4 only without DW4_REGS)
  float gsum[4];
  // float64 loss / advantage sums in registers (lanes kh == 0), folded once after the loop: an
  // LDS read-modify-write per tile put its latency on the loss section's serial chain (-1 %)
  double dsum0, dsum1, dsum2;

  __device__ __forceinline__ void init(const char *Lw, const WaveSlot<G> &ws, int nin_rt = 0,
                                       const double *counts_ = nullptr, double m_global_ = 0.0) {
    const int j = ws.j, kh = ws.kh, G_ = ws.G, q4 = (ws.l >> 2) & 3, p4 = ws.l & 3;
    nin = geo_nin<G>(nin_rt);
    counts = counts_;
    m_global = m_global_;
    // lane address bases: every fragment access is one of these plus a constant
    w1row = Lw + G::O_W1 + j * G::W1_ROWB + 16 * kh;
    w2row = Lw + G::O_W2 + j * W2_ROWB + 8 * kh;
    w3row = Lw + G::O_W3 + j * W3_ROWB + 8 * kh;
    w2tr = Lw + G::O_W2 + (4 * (G_ >> 1) + q4) * W2_ROWB + 8 * (4 * (G_ & 1) + p4);
    w3tr = Lw + G::O_W3 + (4 * (G_ >> 1) + q4) * W3_ROWB + 8 * (4 * (G_ & 1) + p4);
    F = reinterpret_cast<const float *>(Lw + G::O_F);
    b40 = uniform_f(F[G::F_B4]);
    b41 = NOUT == 2 ? uniform_f(F[G::F_B4 + 1]) : 0.0f;
    // loop-invariant weight fragments read from LDS once
    if constexpr (HAND_PLACED) {
      for (int t = 0; t < 2; t++)
        for (int s = 0; s < 2; s++) wf2[t][s] = w_fwd<W2_ROWB, W2_PART>(w2row, t, s);
      for (int s = 0; s < 4; s++) wf3[s] = w_fwd<W3_ROWB, W3_PART>(w3row, 0, s);
    }
    if constexpr (HOLD_BWD) {
      for (int t = 0; t < 2; t++)
        for (int s = 0; s < 2; s++) wb3[t][s] = w_bwd<W3_ROWB, W3_PART>(w3tr, t, s);
      for (int s = 0; s < 4; s++) wb2[s] = w_bwd<W2_ROWB, W2_PART>(w2tr, 0, s);
    }
    gW2a = zero16(), gW2b = zero16(), gW3a = zero16(), gW3b = zero16();
    for (int c = 0; c < KS1; c++) gW1t[c][0] = gW1t[c][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 4; k++) gsum[k] = 0.f;
    dsum0 = dsum1 = dsum2 = 0.0;
    if constexpr (DW4_REGS) gW4r = zero16();
    gBS = zero16();
    if constexpr (HAND_PLACED) {
      for (int q = 0; q < 3; q++) ea0.p[q] = ea1.p[q] = exb.p[q] = u32x4{0u, 0u, 0u, 0u};
    }
    for (int q = 0; q < 3; q++) {
      const uint32_t v = j == q ? 0x3f803f80u : 0u;
      oh[q] = u32x4{v, v, v, v};
      // opaque (not a rematerialisable constant): the compiler would rebuild it with a
      // v_accvgpr_write right before its MFMA, a write the MFMA reads without wait states
      if constexpr (HAND_PLACED) asm volatile("" : "+a"(oh[q]));
    }
  }
  __device__ __forceinline__ F3 fw2(int t, int s) const {
    if constexpr (HAND_PLACED) return wf2[t][s];
    else return w_fwd<W2_ROWB, W2_PART>(w2row, t, s);
  }
  __device__ __forceinline__ F3 fw3(int s) const {
    if constexpr (HAND_PLACED) return wf3[s];
    else return w_fwd<W3_ROWB, W3_PART>(w3row, 0, s);
  }
  __device__ __forceinline__ F3 bw3(int t, int s) const {
    if constexpr (HOLD_BWD) return wb3[t][s];
    else return w_bwd<W3_ROWB, W3_PART>(w3tr, t, s);
  }
  __device__ __forceinline__ F3 bw2(int s) const {
    if constexpr (HOLD_BWD) return wb2[s];
    else return w_bwd<W2_ROWB, W2_PART>(w2tr, 0, s);
  }

  // One 32-row tile whose inputs sit in `slot` (X [32][13] | ret V | act logp_old).  The critic
  // writes V (rows row0 .. row0 + nrows) to Vout; the actor normalises A = ret - V with
  // (meanf, stdf).
  __device__ __forceinline__ void tile(const WaveSlot<G> &ws, const float *slot, int64_t row0, int nrows,
                                       float *__restrict__ Vout, float meanf, float stdf, double inv_m,
                                       float out_mean, float out_std) {
    const int nin = G::NIC ? G::NIC : this->nin;
    const int l = ws.l, j = ws.j, kh = ws.kh, G_ = ws.G;
    float *T = ws.T;
    char *imw = ws.imw;
    const char *imr = ws.imr, *imr16 = ws.imr16;
    constexpr int O_IM2 = G::O_IM2;
    auto radd = [&](int k, float v) { gsum[k] += v; };
    const float *Xs = slot + G::IN_X;
    // ---- layer 1: h1^T = W1 . [X | 1]^T (b1 rides in input column nin), K-step s = columns 16s..
    auto layer1 = [&]() {
      f32x16 h = zero16();
#pragma unroll
      for (int s = 0; s < KS1; s++) {
        float v8[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
          // row j, input column k = 16s + 8h + q (the bias input at k = nin).  Columns past nin
          // read the next row's first inputs (the slot's last row reads into its s0 block).
          const int k = 16 * s + 8 * kh + q;
          const float v = Xs[j * nin + k];
          v8[q] = k < nin ? v : (k == nin ? 1.0f : 0.0f);
        }
        h = mfma6(rd_pair<G::W1_PART>(w1row + 32 * s, 8), split8(v8), h);
      }
      relu16(h);
      return h;
    };
    f32x16 h1;
    if constexpr (HAND_PLACED) h1 = layer1_s(ws, Xs);
    else h1 = layer1();
    MHPPO_MARK(2);
    // ---- layer 2 (the biases ride in as the chains' initial accumulators)
    f32x16 h2a = feat_vec(F, kh), h2b = feat_vec(F + 32, kh);
    f32x16 h3 = feat_vec(F + 64, kh);
    F3 h1s[2], h2as[2], h2bs[2], xb;  // hand-placed: the forward's splits (kept for the backward's images)
    F3 sha0, sha1;                    // hand-placed: dW3's B operands (the h2a image's reads, in layer 3's shadows)
    if constexpr (HAND_PLACED) {
      fwd_s(ws, Xs, h1, h1s, h2a, h2b, h2as, h2bs, h3, xb, sha0, sha1);
    } else {
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const F3 b = split_step(h1, s);
        h2a = mfma6(fw2(0, s), b, h2a);
        h2b = mfma6(fw2(1, s), b, h2b);
      }
      relu16(h2a);
      relu16(h2b);
      MHPPO_MARK(3);
      // ---- layer 3
#pragma unroll
      for (int s = 0; s < 2; s++) h3 = mfma6(fw3(s), split_step(h2a, s), h3);
#pragma unroll
      for (int s = 0; s < 2; s++) h3 = mfma6(fw3(2 + s), split_step(h2b, s), h3);
    }
    relu16(h3);
    MHPPO_MARK(4);
    // ---- output and loss gradient dL/dy for this lane's row (as the f32 path)
    const f32x16 w4v = feat_vec(F + G::F_W4, kh);
    float part0 = 0.0f;
#pragma unroll
    for (int r = 0; r < 16; r++) part0 = fmaf(w4v[r], h3[r], part0);
    const float y0 = xhalf_sum(part0) + b40;
    f32x16 w4v1;
    float y1 = 0.0f;
    if constexpr (NOUT == 2) {
      w4v1 = feat_vec(F + G::F_W4 + 32, kh);
      float part1 = 0.0f;
#pragma unroll
      for (int r = 0; r < 16; r++) part1 = fmaf(w4v1[r], h3[r], part1);
      y1 = xhalf_sum(part1) + b41;
    }
    const bool valid = j < nrows;
    float dy0 = 0.0f, dy1 = 0.0f;
    if (valid) {
      const float rt = slot[G::IN_S0 + j];
      if constexpr (KIND == K_CRITIC) {
        const float v = y0;
        // the store's range is the tile's rows in the batch (a wrong row index reaches no memory)
        if (kh == 0)
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsrc(Vout + row0, 4 * nrows), 4 * j, 0, 0);
        const float a = rt - v;
        const float d = v - rt;
        if (kh == 0) {
          dsum0 += (double)d * (double)d;
          dsum1 += (double)a;
          dsum2 += (double)a * (double)a;
        }
        dy0 = (float)(2.0 * inv_m * (double)d);
      } else if constexpr (KIND == K_CONT) {
        float t, x;
        const float mu = finish_cont<LibmUpdate>(y0, out_mean, out_std, t);
        const float A = adv_normalised(rt - slot[G::IN_S0 + 32 + j], meanf, stdf);
        const float lp = cont_logp_x(slot[G::IN_S1 + j], mu, x);
        // the ratio's magnitude in float32, its clip branch decided in float64 (see the note at
        // the head of this file)
        const float lpo = slot[G::IN_S1 + 32 + j];
        const float r = expf(lp - lpo);
        float dfdr;
        const float f = surr_and_grad_fd(r, (double)lp - (double)lpo, A, dfdr);
        if (kh == 0) dsum0 += (double)f;
        const float dmu = cont_dmu(inv_m, dfdr, r, x);
        dy0 = (dmu * out_std) * (1.0f - t * t);
      } else {
        // choice actor (train_model_d :818-851): the M x M Categorical broadcast in its O(M) form
        // with the global action counts (or the opt-in per-row loss: the row's own action, weight M)
        float p[2], pn[2];
        softmax_pair<LibmUpdate>(y0, y1, p[0], p[1]);
        const float A = adv_normalised(rt - slot[G::IN_S0 + 32 + j], meanf, stdf);
        const double old = (double)slot[G::IN_S1 + j];
        const float sp = cat_normalise(p[0], p[1], pn);
        const double inv_m2 = inv_m * inv_m;
        const int a_row = counts ? 0 : (int)slot[G::IN_S1 + 32 + j];
        double dlp[2], f = 0.0;
#pragma unroll
        for (int k = 0; k < 2; k++) {  // the body restates ppo_heads.h choice_term (a call compiles to other code)
          const double wk = counts ? counts[k] : (k == a_row ? m_global : 0.0);
          const float pc = pn[k] < CAT_EPS ? CAT_EPS : (pn[k] > CAT_HI ? CAT_HI : pn[k]);
          const double r = exp((double)logf(pc) - old);
          double dfdr;
          const double fk = surr_and_grad(r, (double)A, dfdr);
          if (wk != 0.0) f += wk * fk;  // weight 0 (per-row: the other action) is no term: 0 * inf stays out
          const double pass = (pn[k] >= CAT_EPS && pn[k] <= CAT_HI) ? 1.0 : 0.0;
          dlp[k] = inv_m2 * wk * dfdr * r * pass / (double)pc;  // dL/dpn_k
        }
        if (kh == 0) dsum0 += f;
        double g0, g1;
        cat_grad_p(dlp, pn, sp, g0, g1);
        float d0, d1;  // not dy0 / dy1 themselves: as out-arguments they would stay in memory until the call is inlined
        softmax_jacobian(p, g0, g1, d0, d1);
        dy0 = d0;
        dy1 = d1;
      }
    }
    radd(1, (kh == 0) ? dy0 : 0.0f);
    if constexpr (NOUT == 2) radd(3, (kh == 0) ? dy1 : 0.0f);
    if constexpr (HAND_PLACED) {
      bwd_s(ws, h1, h2a, h2b, h3, w4v, dy0, xb, sha0, sha1);
      return;
    }
    // ---- layer 4 backward: d3 = dH3^T masked; dW4 = row sums of dy h3
    f32x16 g, d3;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      g[r] = dy0 * h3[r];
      if constexpr (NOUT == 2) d3[r] = (h3[r] > 0.0f) ? fmaf(w4v1[r], dy1, w4v[r] * dy0) : 0.0f;
      else d3[r] = (h3[r] > 0.0f) ? w4v[r] * dy0 : 0.0f;
    }
    if constexpr (DW4_REGS) {
#pragma unroll
      for (int r = 0; r < 16; r++) gW4r[r] = fmaf(dy0, h3[r], gW4r[r]);
    } else {
      X3_ROWSUM(0, g);
      if constexpr (NOUT == 2) {
        f32x16 g1;
#pragma unroll
        for (int r = 0; r < 16; r++) g1[r] = dy1 * h3[r];
        X3_ROWSUM(2, g1);
      }
    }
    MHPPO_MARK(5);
    // ---- dW3 = sum over rows of d3 (x) h2: A = d3 image, B = h2a / h2b images
    const F3 d3f0 = split_step(d3, 0), d3f1 = split_step(d3, 1);
    // dH2^T = W3^T . dH3^T (below, or here with DH2_FIRST: issued before the dW3 block)
    f32x16 d2a = zero16(), d2b = zero16();
    auto dh2 = [&]() {
      d2a = mfma6(bw3(0, 0), d3f0, d2a);
      d2a = mfma6(bw3(0, 1), d3f1, d2a);
      d2b = mfma6(bw3(1, 0), d3f0, d2b);
      d2b = mfma6(bw3(1, 1), d3f1, d2b);
    };
    if constexpr (CFG::DH2_FIRST) dh2();
    img_write(imw, d3f0, d3f1);
    lds_order();
    const F3 ad0 = img_read(imr, 0), ad1 = img_read(imr, 1);
    lds_order();
    // h2a to the second image, h2b behind the d3 reads in the first: every later fragment is
    // read in the gaps of the MFMA block before the one that consumes it
    img_write(imw + O_IM2, split_step(h2a, 0), split_step(h2a, 1));
    lds_order();
    const F3 ha0 = img_read(imr + O_IM2, 0);
    lds_order();
    img_write(imw, split_step(h2b, 0), split_step(h2b, 1));
    lds_order();
    {
      F3 ha1, hb0, hb1;
      macc6_rd<false, O_IM2 + 16 * IM_ROWB>(ad0, ha0, gW3a, ha1, imr);
      macc6_rd<true, 0>(ad1, ha1, gW3a, hb0, imr);
      macc6_rd<true, 16 * IM_ROWB>(ad0, hb0, gW3b, hb1, imr);
      macc6_w(ad1, hb1, gW3b);
    }
    macc3(ad0, oh[0], gBS);  // dB3
    macc3(ad1, oh[0], gBS);
    lds_order();
    MHPPO_MARK(6);
    // ---- dH2^T = W3^T . dH3^T, masked by h2 > 0
    if constexpr (!CFG::DH2_FIRST) dh2();
    relu_mask(d2a, h2a);
    relu_mask(d2b, h2b);
    MHPPO_MARK(7);
    // the B operand of dW1's input columns 16c .. 16c + 15: rows 8G .. 8G + 7 of column 16c + n
    auto xcols = [&](int c) {
      float xv[8];
      const int n = 16 * c + (l & 15);
#pragma unroll
      for (int q = 0; q < 8; q++) {
        const float v = Xs[(8 * G_ + q) * nin + (n < nin ? n : 0)];
        xv[q] = n < nin ? v : (n == nin ? 1.0f : 0.0f);
      }
      return split8(xv);
    };
    // ---- dH1^T = W2^T . dH2^T, masked by h1 > 0; dW2 = sum over rows of d2 (x) h1
    f32x16 d1 = zero16();
    const F3 f0 = split_step(d2a, 0), f1 = split_step(d2a, 1);
    d1 = mfma6(bw2(0), f0, d1);
    d1 = mfma6(bw2(1), f1, d1);
    // B = h1 image (second slot), A = d2a image (first slot), then d2b into the second slot
    // behind the h1 reads; the A fragments after the first are read in the MFMA gaps
    img_write(imw + O_IM2, split_step(h1, 0), split_step(h1, 1));
    lds_order();
    const F3 bh0 = img_read(imr + O_IM2, 0), bh1 = img_read(imr + O_IM2, 1);
    lds_order();
    img_write(imw, f0, f1);
    lds_order();
    const F3 f2 = split_step(d2b, 0), f3 = split_step(d2b, 1);
    img_write(imw + O_IM2, f2, f3);
    lds_order();
    d1 = mfma6(bw2(2), f2, d1);
    d1 = mfma6(bw2(3), f3, d1);
    const F3 da0 = img_read(imr, 0);
    lds_order();
    {
      F3 da1, db0, db1;
      macc6_rd<false, 16 * IM_ROWB>(da0, bh0, gW2a, da1, imr);
      macc6_rd<true, O_IM2>(da1, bh1, gW2a, db0, imr);
      macc6_rd<true, O_IM2 + 16 * IM_ROWB>(db0, bh0, gW2b, db1, imr);
      macc6_w(db1, bh1, gW2b);
      // dB2; every fragment complete: macc6_w waited for db1, the blocks before for the rest
      macc3(da0, oh[1], gBS);
      macc3(da1, oh[1], gBS);
      macc3(db0, oh[2], gBS);
      macc3(db1, oh[2], gBS);
    }
    lds_order();
    relu_mask(d1, h1);
    MHPPO_MARK(8);
    // ---- dW1 = sum over rows of d1 (x) [X | 1]: A = d1 image, B = the input rows (column 13:
    // the constant 1, i.e. dB1).  16x16x32 tiles (out features 16t..16t+15 x input columns
    // 0..15, all 32 rows in one K-step): lane l of group G = l >> 4 holds rows 8G..8G+7 of
    // column l & 15 / feature l & 15
    img_write(imw, split_step(d1, 0), split_step(d1, 1));
    lds_order();
    {
      const F3 b = xcols(0);
      const F3 a0 = tr_pair<IM_PART>(imr16, 4 * IM_ROWB);
      F3 a1;
      macc6_16_rd<false, 32>(a0, b, gW1t[0][0], a1, imr16);
      macc6_16_w(a1, b, gW1t[0][1]);
#pragma unroll
      for (int c = 1; c < KS1; c++) {
        const F3 bc = xcols(c);
        macc6_16(a0, bc, gW1t[c][0]);
        macc6_16(a1, bc, gW1t[c][1]);
      }
    }
    lds_order();
    MHPPO_MARK(9);
  }

  // The previous tile's dW1 block E: 12 AGPR MFMAs (16x16x32) on the deferred operands
  template <int K>
  __device__ __forceinline__ void mac_e() {
    constexpr int P = K % 6;
    if constexpr (K < 6) mac1_16(ea0.p[P6A[P]], exb.p[P6B[P]], gW1t[0][0]);
    else mac1_16(ea1.p[P6A[P]], exb.p[P6B[P]], gW1t[0][1]);
  }
  // Layer 1 of one tile, hand-placed, with the PREVIOUS tile's dW1 block in its shadows: the
  // input loads first, then E's MFMAs carry the input split, then layer 1's six MFMAs alternate with
  // E's last ones.  (E used to end the tile: twelve 16-cycle MFMAs with nothing beside them, behind
  // the LDS latency of their operand reads; deferred, its operands are already in registers.)  The
  // per-accumulator product order is unchanged: the same bits.  Returns ReLU(h1).
  __device__ __forceinline__ f32x16 layer1_s(const WaveSlot<G> &ws, const float *Xs) {
    const int j = ws.j, kh = ws.kh;
    float v8[8], rs[8];
#pragma unroll
    for (int q = 0; q < 8; q++) v8[q] = Xs[j * NIN_CONT + 8 * kh + q];  // past column 12: unused
    pin4(v8);
    pin4(v8 + 4);
#pragma unroll
    for (int q = 0; q < 8; q++) {  // row j, input column 8h + q (the bias input at column 13)
      const int k = 8 * kh + q;
      v8[q] = k < NIN_CONT ? v8[q] : (k == NIN_CONT ? 1.0f : 0.0f);
    }
    const F3 w1 = rd_pair<G::W1_PART>(w1row, 8);
    F3 xs;
    f32x16 h = zero16();
    // regions: E0 E1 | E2..E9 + the input split | L0 E10 L1 E11 L2 L3 L4 L5
    constexpr int ORD[18] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 100, 10, 101, 11, 102, 103, 104, 105};
    weave<18, Plan<2, 10, 8>>(
        [&](auto kc) {
          constexpr int K = decltype(kc)::value, M = ORD[K];
          if constexpr (M < 100) mac_e<M>();
          else h = mfma_b(w1.p[P6A[M - 100]], xs.p[P6B[M - 100]], h);
        },
        [&](auto uc) {
          constexpr int U = decltype(uc)::value;
          if constexpr (U % 2 == 0) split_l1(v8, U / 2, xs, rs);
          else split_l2(U / 2, xs, rs);
        });
    relu16(h);
    return h;
  }
  // after the tile loop: the last tile's deferred dW1 block (once per launch: every MFMA behind
  // enough wait states for a compiler copy of its accumulator or operands just before it)
  __device__ __forceinline__ void drain() {
    if constexpr (HAND_PLACED) {
      sfor<0, 12>([&](auto kc) {
        constexpr int K = decltype(kc)::value, P = K % 6;
        f32x4 &c = K < 6 ? gW1t[0][0] : gW1t[0][1];
        const F3 &a = K < 6 ? ea0 : ea1;
        asm volatile("s_nop 4\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a.p[P6A[P]]), "v"(exb.p[P6B[P]]));
      });
    }
  }

  // Layers 2 and 3 of one tile, hand-placed: each layer's MFMAs carry the splits its own later
  // K-steps and the next layer need (the same products in the same order per accumulator as the
  // plain forward, so the same bits):
  //   L2  [h2a s0 | h2a s1 | h2b s0 | h2b s1]  | h1's K-step 1 split, dW1's input-column split,
  //                                              h2a's ReLU and split (after its last MFMA)
  //   L3  [h2a s0 | h2a s1 | h2b s0 | h2b s1]  | the rest of h2a's split, h2b's ReLU and split
  // h1 arrives ReLU'd; h2a / h2b / h3 leave as the layers' pre-ReLU accumulators for h3 (the caller
  // applies its ReLU) and ReLU'd for h2a / h2b.
  __device__ __forceinline__ void fwd_s(const WaveSlot<G> &ws, const float *Xs, const f32x16 &h1, F3 (&h1s)[2],
                                        f32x16 &h2a, f32x16 &h2b, F3 (&h2as)[2], F3 (&h2bs)[2], f32x16 &h3,
                                        F3 &xb, F3 &ha0, F3 &ha1) {
    const int l = ws.l, G_ = ws.G;
    char *imw = ws.imw;
    const char *imr = ws.imr;
    constexpr int RS = 16 * IM_ROWB, DU = 4 * IM_ROWB;
    float rs[8], rt[8], xv[8];
    float h1v[16];
#pragma unroll
    for (int r = 0; r < 16; r++) h1v[r] = h1[r];
#pragma unroll
    for (int q = 0; q < 4; q++) split_l1(h1v, q, h1s[0], rs);
#pragma unroll
    for (int q = 0; q < 4; q++) split_l2(q, h1s[0], rs);
    {
      const F3 w00 = fw2(0, 0), w01 = fw2(0, 1), w10 = fw2(1, 0), w11 = fw2(1, 1);
      // h1 s1 split (8 units, before k = 6), dW1's B operand (1 + 8), h2a ReLU (4, after its last
      // MFMA k = 11 has landed) + h2a s0 split (8) + h2a s1 split level 1 (4); the h1 image (slot 3,
      // six stores, one per two shadows; its K-step 1 half after that split)
      using PL = Plan<0, 5, 8, 5, 12, 10, 13, 24, 16, 1, 13, 6>;
      static_assert(PL::reg(7) < 6 && PL::reg(7) < PL::reg(37), "h1's K-step 1 before its MFMAs and its image");
      weave<24, PL>(
          [&](auto kc) {
            constexpr int K = decltype(kc)::value, P = K % 6, T = K / 6;
            if constexpr (T == 0) h2a = mfma_b(w00.p[P6A[P]], h1s[0].p[P6B[P]], h2a);
            if constexpr (T == 1) h2a = mfma_b(w01.p[P6A[P]], h1s[1].p[P6B[P]], h2a);
            if constexpr (T == 2) h2b = mfma_b(w10.p[P6A[P]], h1s[0].p[P6B[P]], h2b);
            if constexpr (T == 3) h2b = mfma_b(w11.p[P6A[P]], h1s[1].p[P6B[P]], h2b);
          },
          [&](auto uc) {
            constexpr int U = decltype(uc)::value;
            if constexpr (U < 8) {
              if constexpr (U % 2 == 0) split_l1(h1v + 8, U / 2, h1s[1], rs);
              else split_l2(U / 2, h1s[1], rs);
            } else if constexpr (U < 10) {  // dW1's B operand: rows 8G .. 8G + 7 of input column l & 15
              const int n = l & 15, nc = n < NIN_CONT ? n : NIN_CONT - 1;
              float v[4];
#pragma unroll
              for (int q = 0; q < 4; q++) v[q] = Xs[(8 * G_ + 4 * (U - 8) + q) * NIN_CONT + nc];
              pin4(v);
#pragma unroll
              for (int q = 0; q < 4; q++) xv[4 * (U - 8) + q] = n < NIN_CONT ? v[q] : (n == NIN_CONT ? 1.0f : 0.0f);
            } else if constexpr (U < 18) {
              constexpr int V = U - 10;
              if constexpr (V % 2 == 0) split_l1(xv, V / 2, xb, rt);
              else split_l2(V / 2, xb, rt);
            } else if constexpr (U < 22) {  // h2a's ReLU
              relu4(h2a, 4 * (U - 18));
            } else if constexpr (U < 30) {  // h2a K-step 0 split
              constexpr int V = U - 22;
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; e++) v[e] = h2a[e];
              if constexpr (V % 2 == 0) split_l1(v, V / 2, h2as[0], rs);
              else split_l2(V / 2, h2as[0], rs);
            } else if constexpr (U < 34) {  // h2a K-step 1 split, level 1 (level 2 in L3)
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; e++) v[e] = h2a[8 + e];
              split_l1(v, U - 30, h2as[1], rt);
            } else {  // the h1 image (slot 3): part (U - 34) % 3 of K-step half (U - 34) / 3
              constexpr int V = U - 34;
              img_write_h(imw + G::O_IM3, h1s[V / 3], V % 3, V / 3);
              lds_order();
            }
          });
    }
    MHPPO_MARK(3);
    {
      const F3 w0 = fw3(0), w1 = fw3(1), w2 = fw3(2), w3 = fw3(3);
      // h2a s1 level 2 (4, before k = 6) + h2b ReLU 0-7 (2) + h2b s0 level 1 (4); h2b s0 level 2 (4,
      // before k = 12) + h2b ReLU 8-15 (2) + h2b s1 level 1 (4); h2b s1 level 2 (4, before k = 18);
      // the h2a image (slot 4) and the h2b image (slot 2), one store per two shadows, each half after
      // its split; the h2a image's transposed reads (dW3's B operands) behind its stores
      using PL = Plan<0, 6, 10, 6, 12, 10, 12, 18, 4, 1, 13, 6, 13, 25, 6, 12, 24, 6>;
      static_assert(PL::reg(3) < 6 && PL::reg(13) < 12 && PL::reg(23) < 18, "splits before their MFMAs");
      static_assert(PL::reg(3) < PL::reg(27) && PL::reg(13) < PL::reg(30) && PL::reg(23) < PL::reg(33) &&
                        PL::reg(29) < PL::reg(36),
                    "image halves after their splits, reads after the stores");
      weave<24, PL>(
          [&](auto kc) {
            constexpr int K = decltype(kc)::value, P = K % 6, T = K / 6;
            if constexpr (T == 0) h3 = mfma_b(w0.p[P6A[P]], h2as[0].p[P6B[P]], h3);
            if constexpr (T == 1) h3 = mfma_b(w1.p[P6A[P]], h2as[1].p[P6B[P]], h3);
            if constexpr (T == 2) h3 = mfma_b(w2.p[P6A[P]], h2bs[0].p[P6B[P]], h3);
            if constexpr (T == 3) h3 = mfma_b(w3.p[P6A[P]], h2bs[1].p[P6B[P]], h3);
          },
          [&](auto uc) {
            constexpr int U = decltype(uc)::value;
            if constexpr (U < 4) {
              split_l2(U, h2as[1], rt);
            } else if constexpr (U < 6) {  // h2b's ReLU, elements 0-7
              relu4(h2b, 4 * (U - 4));
            } else if constexpr (U < 10) {
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; e++) v[e] = h2b[e];
              split_l1(v, U - 6, h2bs[0], rs);
            } else if constexpr (U < 14) {
              split_l2(U - 10, h2bs[0], rs);
            } else if constexpr (U < 16) {  // h2b's ReLU, elements 8-15
              relu4(h2b, 8 + 4 * (U - 14));
            } else if constexpr (U < 20) {
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; e++) v[e] = h2b[8 + e];
              split_l1(v, U - 16, h2bs[1], rt);
            } else if constexpr (U < 24) {
              split_l2(U - 20, h2bs[1], rt);
            } else if constexpr (U < 30) {  // the h2a image (slot 4)
              constexpr int V = U - 24;
              img_write_h(imw + G::O_IM4, h2as[V / 3], V % 3, V / 3);
              lds_order();
            } else if constexpr (U < 36) {  // the h2b image (slot 2: the previous tile's d2b reads are issued)
              constexpr int V = U - 30;
              img_write_h(imw + G::O_IM2, h2bs[V / 3], V % 3, V / 3);
              lds_order();
            } else if constexpr (U < 39) {
              tr_pt(imr + G::O_IM4, DU, U - 36, ha0);
            } else {
              tr_pt(imr + G::O_IM4 + RS, DU, U - 39, ha1);
              lds_order();
            }
          });
    }
  }

  // The backward of one tile, hand-placed: five MFMA blocks, each carrying the work the
  // next block needs in its MFMA shadows (the plans below place it).  An image goes out as six
  // single stores at most one per two shadows (img_write_h: LDS stores, not the MFMAs, otherwise set
  // the pace), its reads one part (two ds_read_b64_tr_b16) per unit:
  //   A  dH2 = W3^T d3      24 on-chain MFMAs | d3's K-step-1 split, the d3 image and its reads, dW4 sums
  //   B  dW3 (+ dB3)        30 AGPR MFMAs     | the h2b image reads, d2a / d2b masks, d2a's split
  //   C  dH1 = W2^T d2      24 on-chain MFMAs | d2b's split, the d2a / d2b images, the h1 / d2a reads
  //   D  dW2 (+ dB2)        36 AGPR MFMAs     | the d2 image reads, d1's mask and split, d1's image
  //                                             and dW1's operand reads
  //   E  dW1 (+ dB1)        12 AGPR MFMAs (16x16x32), deferred into the next tile's layer 1
  // The forward wrote the h1 (slot 3), h2a (slot 4) and h2b (slot 2) images and read h2a's (ha0,
  // ha1).  Slot 1: d3, then d2a, then d1; slot 2: h2b, then d2b.  The same products in the same order
  // per accumulator as the phase-by-phase backward (the same bits); an image slot is rewritten only
  // after its last reads were issued (a wave's LDS operations execute in order).  xb: dW1's B operand
  // (input columns), split in the forward.
  __device__ __forceinline__ void bwd_s(const WaveSlot<G> &ws, const f32x16 &h1, const f32x16 &h2a, const f32x16 &h2b,
                                        const f32x16 &h3, const f32x16 &w4v, float dy0, const F3 &xb, const F3 &ha0,
                                        const F3 &ha1) {
    char *imw = ws.imw;
    const char *imr = ws.imr, *imr16 = ws.imr16;
    constexpr int O_IM2 = G::O_IM2, O_IM3 = G::O_IM3, RS = 16 * IM_ROWB, DU = 4 * IM_ROWB;  // K-step 1 rows; tr_pair stride
    // d3 = dH3 masked by h3 > 0 (on the chain); its K-step 0 split here, K-step 1 in block A
    float d3[16];
#pragma unroll
    for (int r = 0; r < 16; r++) d3[r] = (h3[r] > 0.0f) ? w4v[r] * dy0 : 0.0f;
    F3 d3f0, d3f1;
    float rs[8];  // the level-1 residuals of the split in progress
#pragma unroll
    for (int q = 0; q < 4; q++) split_l1(d3, q, d3f0, rs);
#pragma unroll
    for (int q = 0; q < 4; q++) split_l2(q, d3f0, rs);
    MHPPO_MARK(5);
    f32x16 d2a = zero16(), d2b = zero16(), d1 = zero16();
    F3 ad0, ad1, hb0, hb1;
    // ---- block A: dH2^T = W3^T dH3^T, K-step 0 of both output tiles first (d3f1 is split meanwhile)
    {
      const F3 w00 = bw3(0, 0), w10 = bw3(1, 0), w01 = bw3(0, 1), w11 = bw3(1, 1);
      // d3f1 split (8), the d3 image (K-step 0 half in 1 3 5, K-step 1 half in 9 11 13), its reads
      // (14 .. 19), dW4 (20 .. 23)
      using PL = Plan<0, 8, 8, 1, 7, 3, 9, 15, 3, 14, 20, 6, 20, 24, 4>;
      static_assert(PL::reg(7) < PL::reg(11) && PL::reg(13) < PL::reg(14), "split, then stores, then reads");
      weave<24, PL>(
          [&](auto kc) {
            constexpr int K = decltype(kc)::value, P = K % 6, T = K / 6;
            if constexpr (T == 0) d2a = mfma_b(w00.p[P6A[P]], d3f0.p[P6B[P]], d2a);
            if constexpr (T == 1) d2b = mfma_b(w10.p[P6A[P]], d3f0.p[P6B[P]], d2b);
            if constexpr (T == 2) d2a = mfma_b(w01.p[P6A[P]], d3f1.p[P6B[P]], d2a);
            if constexpr (T == 3) d2b = mfma_b(w11.p[P6A[P]], d3f1.p[P6B[P]], d2b);
          },
          [&](auto uc) {
            constexpr int U = decltype(uc)::value;
            if constexpr (U < 8) {  // d3's K-step 1 split
              if constexpr (U % 2 == 0) split_l1(d3 + 8, U / 2, d3f1, rs);
              else split_l2(U / 2, d3f1, rs);
            } else if constexpr (U < 14) {  // the d3 image (slot 1: the previous tile's d1 reads are issued)
              constexpr int V = U - 8;
              img_write_h(imw, V < 3 ? d3f0 : d3f1, V % 3, V / 3);
              lds_order();
            } else if constexpr (U < 17) {
              tr_pt(imr, DU, U - 14, ad0);
            } else if constexpr (U < 20) {
              tr_pt(imr + RS, DU, U - 17, ad1);
              lds_order();
            } else {  // dW4: sum over rows of dy h3, per lane and register
#pragma unroll
              for (int r = 4 * (U - 20); r < 4 * (U - 19); r++) gW4r[r] = fmaf(dy0, h3[r], gW4r[r]);
            }
          });
    }
    MHPPO_MARK(6);
    // ---- block B: dW3 = sum over rows of d3 (x) h2 (A = the d3 image, B = the h2a / h2b images), dB3
    F3 f0, f1;  // d2a's split (block C's first operands)
    {
      using PL = Plan<0, 6, 6, 6, 30, 32>;
      static_assert(PL::reg(2) < 12 && PL::reg(5) < 18, "image reads before their MFMAs");
      weave<30, PL>(
          [&](auto kc) {
            constexpr int K = decltype(kc)::value, P = K % 6, T = K / 6;
            if constexpr (T == 0) mac1(ad0.p[P6A[P]], ha0.p[P6B[P]], gW3a);
            if constexpr (T == 1) mac1(ad1.p[P6A[P]], ha1.p[P6B[P]], gW3a);
            if constexpr (T == 2) mac1(ad0.p[P6A[P]], hb0.p[P6B[P]], gW3b);
            if constexpr (T == 3) mac1(ad1.p[P6A[P]], hb1.p[P6B[P]], gW3b);
            if constexpr (T == 4) mac1_oh((P < 3 ? ad0 : ad1).p[2 - P % 3], oh[0], gBS);
          },
          [&](auto uc) {
            constexpr int U = decltype(uc)::value;
            if constexpr (U < 3) {  // the h2b image (slot 2, written in layer 3)
              tr_pt(imr + O_IM2, DU, U, hb0);
            } else if constexpr (U < 6) {
              tr_pt(imr + O_IM2 + RS, DU, U - 3, hb1);
              lds_order();
            } else if constexpr (U < 14) {  // d2a masked by h2a > 0, two elements per unit
              mask2(d2a, h2a, 2 * (U - 6));
            } else if constexpr (U < 30) {  // d2a's split: K-step 0 -> f0, 1 -> f1
              constexpr int V = U - 14, st = V / 8, q = (V % 8) / 2;
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; e++) v[e] = d2a[8 * st + e];
              if constexpr (V % 2 == 0) split_l1(v, q, st ? f1 : f0, rs);
              else split_l2(q, st ? f1 : f0, rs);
            } else {  // d2b masked by h2b > 0 (block A's last MFMAs have landed by now)
              mask2(d2b, h2b, 2 * (U - 30));
            }
          });
    }
    MHPPO_MARK(7);
    // ---- block C: dH1^T = W2^T dH2^T (one accumulator chain over the four K-steps)
    F3 f2, f3, bh0, bh1, da0;
    {
      const F3 w0 = bw2(0), w1 = bw2(1), w2 = bw2(2), w3 = bw2(3);
      // d2b's split (K-step 0 in 0 .. 10, 1 in 11 .. 16), the d2a image (0 2 .. 10, slot 1: the d3
      // reads are issued) and the d2b image (12 14 .. 22, slot 2: the h2b reads are issued), the h1
      // image reads (1 .. 11), d2a's first reads (13 15 17)
      using PL = Plan<0, 11, 8, 11, 17, 8, 0, 12, 6, 12, 24, 6, 1, 7, 3, 7, 13, 3, 13, 19, 3>;
      static_assert(PL::reg(7) < 12 && PL::reg(15) < 18, "d2b's split before its MFMAs");
      static_assert(PL::reg(7) < PL::reg(22) && PL::reg(15) < PL::reg(25) && PL::reg(21) < PL::reg(34),
                    "image halves after their splits, reads after the stores");
      weave<24, PL>(
          [&](auto kc) {
            constexpr int K = decltype(kc)::value, P = K % 6, T = K / 6;
            if constexpr (T == 0) d1 = mfma_b(w0.p[P6A[P]], f0.p[P6B[P]], d1);
            if constexpr (T == 1) d1 = mfma_b(w1.p[P6A[P]], f1.p[P6B[P]], d1);
            if constexpr (T == 2) d1 = mfma_b(w2.p[P6A[P]], f2.p[P6B[P]], d1);
            if constexpr (T == 3) d1 = mfma_b(w3.p[P6A[P]], f3.p[P6B[P]], d1);
          },
          [&](auto uc) {
            constexpr int U = decltype(uc)::value;
            auto split_d2b = [&](int st, int V) {  // d2b's split: K-step 0 -> f2, 1 -> f3
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; e++) v[e] = d2b[8 * st + e];
              if (V % 2 == 0) split_l1(v, V / 2, st ? f3 : f2, rs);
              else split_l2(V / 2, st ? f3 : f2, rs);
            };
            if constexpr (U < 8) {
              split_d2b(0, U);
            } else if constexpr (U < 16) {
              split_d2b(1, U - 8);
            } else if constexpr (U < 22) {  // the d2a image (slot 1)
              constexpr int V = U - 16;
              img_write_h(imw, V < 3 ? f0 : f1, V % 3, V / 3);
              lds_order();
            } else if constexpr (U < 28) {  // the d2b image (slot 2)
              constexpr int V = U - 22;
              img_write_h(imw + O_IM2, V < 3 ? f2 : f3, V % 3, V / 3);
              lds_order();
            } else if constexpr (U < 31) {  // the h1 image (slot 3, written in layer 2)
              tr_pt(imr + O_IM3, DU, U - 28, bh0);
            } else if constexpr (U < 34) {
              tr_pt(imr + O_IM3 + RS, DU, U - 31, bh1);
            } else {
              tr_pt(imr, DU, U - 34, da0);
              lds_order();
            }
          });
    }
    MHPPO_MARK(8);
    // ---- block D: dW2 = sum over rows of d2 (x) h1 (A = the d2a / d2b images, B = the h1 image), dB2
    F3 a0, a1;
    {
      F3 da1, db0, db1, e0, e1;
      // the d2 reads (0 .. 8), d1's mask (2 .. 9, after block C's last MFMA has landed) and split
      // (10 .. 25), the d1 image (19 21 23 | 27 29 31, slot 1: the d2a reads are issued), dW1's
      // operand reads (32 .. 35)
      using PL = Plan<0, 9, 9, 2, 10, 8, 10, 26, 16, 19, 25, 3, 27, 33, 3, 32, 36, 6>;
      static_assert(PL::reg(2) < 6 && PL::reg(5) < 12 && PL::reg(8) < 18, "image reads before their MFMAs");
      static_assert(PL::reg(24) < PL::reg(33) && PL::reg(32) < PL::reg(36) && PL::reg(38) < PL::reg(39),
                    "image halves after their splits, reads after the stores");
      weave<36, PL>(
          [&](auto kc) {
            constexpr int K = decltype(kc)::value, P = K % 6, T = K / 6;
            if constexpr (T == 0) mac1(da0.p[P6A[P]], bh0.p[P6B[P]], gW2a);
            if constexpr (T == 1) mac1(da1.p[P6A[P]], bh1.p[P6B[P]], gW2a);
            if constexpr (T == 2) mac1(db0.p[P6A[P]], bh0.p[P6B[P]], gW2b);
            if constexpr (T == 3) mac1(db1.p[P6A[P]], bh1.p[P6B[P]], gW2b);
            if constexpr (T == 4) mac1_oh((P < 3 ? da0 : da1).p[2 - P % 3], oh[1], gBS);
            if constexpr (T == 5) mac1_oh((P < 3 ? db0 : db1).p[2 - P % 3], oh[2], gBS);
          },
          [&](auto uc) {
            constexpr int U = decltype(uc)::value;
            if constexpr (U < 3) {
              tr_pt(imr + RS, DU, U, da1);
              lds_order();
            } else if constexpr (U < 6) {
              tr_pt(imr + O_IM2, DU, U - 3, db0);
            } else if constexpr (U < 9) {
              tr_pt(imr + O_IM2 + RS, DU, U - 6, db1);
            } else if constexpr (U < 17) {  // d1 masked by h1 > 0
              mask2(d1, h1, 2 * (U - 9));
            } else if constexpr (U < 33) {  // d1's split -> e0, e1
              constexpr int V = U - 17, st = V / 8, q = (V % 8) / 2;
              float v[8];
#pragma unroll
              for (int e = 0; e < 8; e++) v[e] = d1[8 * st + e];
              if constexpr (V % 2 == 0) split_l1(v, q, st ? e1 : e0, rs);
              else split_l2(q, st ? e1 : e0, rs);
            } else if constexpr (U < 39) {  // the d1 image (slot 1)
              constexpr int V = U - 33;
              img_write_h(imw, V < 3 ? e0 : e1, V % 3, V / 3);
              lds_order();
            } else if constexpr (U < 42) {  // dW1's A operands: 16x16x32 transposed reads
              tr_pt(imr16, DU, U - 39, a0);
            } else {
              tr_pt(imr16 + 32, DU, U - 42, a1);
            }
          });
    }
    MHPPO_MARK(9);
    // ---- block E: dW1 = sum over rows of d1 (x) [X | 1] (column 13: dB1), two 16x16x32 tiles,
    // deferred into the next tile's layer-1 shadows (layer1_s; the last tile's: drain)
    ea0 = a0;
    ea1 = a1;
    exb = xb;
    lds_order();
  }

  // this wave's partial gradient (packed torch layout) and float64 sums
  __device__ __forceinline__ void finish(const WaveSlot<G> &ws, float *__restrict__ gp, double *__restrict__ dp) {
    const int nin = G::NIC ? G::NIC : this->nin;
    const Packed P(nin, NOUT);
    const int l = ws.l, j = ws.j, kh = ws.kh, G_ = ws.G;
    if constexpr (KS1 == 1) macc_drain(gW2a, gW2b, gW3a, gW3b, gW1t[0][0], gW1t[0][1]);
    else macc_drain2(gW2a, gW2b, gW3a, gW3b, gW1t[0][0], gW1t[0][1], gW1t[KS1 - 1][0], gW1t[KS1 - 1][1]);
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" : "+a"(gBS));
    float gW4 = gsum[0], gB4 = gsum[1], gW41 = gsum[2], gB41 = gsum[3];
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int f = feat(r, l);
      gp[P.W2 + f * 32 + j] = gW2a[r];
      gp[P.W2 + (32 + f) * 32 + j] = gW2b[r];
      gp[P.W3 + f * 64 + j] = gW3a[r];
      gp[P.W3 + f * 64 + 32 + j] = gW3b[r];
    }
#pragma unroll
    for (int c = 0; c < KS1; c++) {
#pragma unroll
      for (int t = 0; t < 2; t++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int f = 16 * t + 4 * G_ + r, n = 16 * c + (l & 15);
          if (n < nin) gp[P.W1 + f * nin + n] = gW1t[c][t][r];
          if (n == nin) gp[P.B1 + f] = gW1t[c][t][r];
        }
      }
    }
    if constexpr (!DW4_REGS) {  // halves of the row sums: lanes j and j + 32 hold rows 0-15 / 16-31 of feature j
      gW4 += __shfl_xor(gW4, 32);
      if (NOUT == 2) gW41 += __shfl_xor(gW41, 32);
      if (kh == 0) {
        gp[P.W4 + j] = gW4;
        if (NOUT == 2) gp[P.W4 + 32 + j] = gW41;
      }
    } else {  // register r of lane (row j, half kh) holds feature feat(r, l): sum over j
#pragma unroll
      for (int r = 0; r < 16; r++) {
        float v = gW4r[r];
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o);
        if (j == 0) gp[P.W4 + feat(r, l)] = v;
      }
    }
    if (j < 3) {  // column q of the row-sum accumulator gBS: lanes q, q + 32 (rows: feat(r, l))
      const int base = j == 0 ? P.B3 : (j == 1 ? P.B2 : P.B2 + 32);
#pragma unroll
      for (int r = 0; r < 16; r++) gp[base + feat(r, l)] = gBS[r];
    }
    float b4s0 = gB4, b4s1 = gB41;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      b4s0 += __shfl_xor(b4s0, o);
      if (NOUT == 2) b4s1 += __shfl_xor(b4s1, o);
    }
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (kh == 0) s0 = dsum0, s1 = dsum1, s2 = dsum2;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s0 += __shfl_xor(s0, o);
      s1 += __shfl_xor(s1, o);
      s2 += __shfl_xor(s2, o);
    }
    if (l == 0) {
      gp[P.B4] = b4s0;
      if (NOUT == 2) gp[P.B4 + 1] = b4s1;
      dp[0] = s0;
      dp[1] = s1;
      dp[2] = s2;
    }
  }
};

// the normalisation of the actor's advantage from the critic pass's global sums: ppo_heads.h
// adv_moments, restated (each moment is made wave-uniform as it is rounded)
__device__ __forceinline__ void adv_norm(const double *stats, double m_global, float &meanf, float &stdf) {
  double mean = stats[0] / m_global;
  double var = (stats[1] - stats[0] * mean) / (m_global - 1.0);
  meanf = uniform_f((float)mean);
  stdf = uniform_f((float)sqrt(var > 0 ? var : 0.0));
}

// Tile inputs of a runtime-width geometry (the choice heads): the X rows as whole 1-KiB LDS-DMA
// pieces (unmasked: buffer loads past the tile's rows return zeros, which land inside the X
// region), s0 = [ret | V], s1 = [logp_old | action] (K_CHOICE; the action only in per-row mode,
// else the lanes re-read logp_old: the same instruction count either way).
template <int KIND, class G>
__device__ __forceinline__ void prefetch_g(float *slot, const float *X, int nin, const float *ret, const float *V,
                                           const float *act, const float *lp, int64_t row0, int l, int64_t M) {
  const uint32_t rows = tile_rows(M, row0);
  const v4i rx = rsrc_v(X + row0 * nin, rows * nin * 4);
#pragma unroll
  for (int c = 0; c < G::XPIECES; c++) dma16(rx, slot + G::IN_X + 256 * c, 1024 * c + 16 * l);
  const uint32_t vo = 4 * (l & 31);
  if (l < 32) dma4(rsrc_v(ret + row0, 4 * rows), slot + G::IN_S0, vo);
  if (KIND != K_CRITIC) {
    if (l >= 32) dma4(rsrc_v(V + row0, 4 * rows), slot + G::IN_S0, vo);
    if (l < 32) dma4(rsrc_v(lp + row0, 4 * rows), slot + G::IN_S1, vo);
    if (l >= 32) dma4(rsrc_v((act ? act : lp) + row0, 4 * rows), slot + G::IN_S1, vo);
  }
}
template <int KIND, class G>
constexpr int prefetch_g_ops() { return G::XPIECES + (KIND == K_CRITIC ? 1 : 4); }

template <int KIND, class G>
__device__ __forceinline__ void load_sync_g(float *slot, const float *X, int nin, const float *ret, const float *V,
                                            const float *act, const float *lp, int64_t row0, int nrows, int l) {
  constexpr int NX = G::XMAX / 64;
  static_assert(G::XMAX % 64 == 0, "X region");
  const auto rx = rsrc(X + row0 * nin, (uint32_t)(nrows * nin) * 4);
  float x[NX];
#pragma unroll
  for (int i = 0; i < NX; i++) x[i] = bload(rx, 4 * (l + 64 * i));  // past the rows: 0
  const uint32_t nb = 4 * nrows, vo = 4 * (l & 31);
  const float s0 = bload(rsrc((l < 32 || KIND == K_CRITIC) ? ret + row0 : V + row0, nb), vo);
  float s1 = 0.0f;
  if (KIND != K_CRITIC) s1 = bload(rsrc((l < 32 || act == nullptr) ? lp + row0 : act + row0, nb), vo);
#pragma unroll
  for (int i = 0; i < NX; i++) slot[G::IN_X + l + 64 * i] = x[i];
  slot[G::IN_S0 + l] = s0;
  slot[G::IN_S1 + l] = s1;
}

// Inputs of this wave's tiles: LDS-DMA one tile ahead into the double-buffered slot; the ragged
// last tile loads synchronously.  body(slot, row0, nrows) runs each tile.  (Two tiles ahead in a
// three-slot ring measured no faster: 1.764 / 1.867-1.871 ms vs 1.749-1.776 / 1.869-1.871 ms per
// critic / actor launch, profiles/r04_x3_probe/ab_pf2.txt.)
template <int KIND, class G>
__device__ __forceinline__ void prefetch_any(const WaveSlot<G> &ws, float *slot, int64_t row0, const float *X, int nin,
                                             const float *ret, const float *V, const float *act, const float *lp_old,
                                             int64_t M) {
  if constexpr (G::NIC == NIN_CONT) prefetch_tile<KIND, LY>(slot, X, ret, V, act, lp_old, row0, ws.l, M);
  else prefetch_g<KIND, G>(slot, X, nin, ret, V, act, lp_old, row0, ws.l, M);
}
// The first tile's LDS-DMA, issued by the kernel before it stages the weights (its own slot is
// disjoint from the weight images), so the HBM latency of the first inputs overlaps the staging;
// tile_loop(..., first_issued = true) then skips it.
template <int KIND, class G>
__device__ __forceinline__ void prefetch_first(const WaveSlot<G> &ws, int64_t gw, int64_t M, const float *X, int nin,
                                               const float *ret, const float *V, const float *act,
                                               const float *lp_old) {
  if (gw < uniform_i64(M / 32)) prefetch_any<KIND, G>(ws, ws.inb, gw * 32, X, nin, ret, V, act, lp_old, M);
}

template <int KIND, class G, class Body>
__device__ __forceinline__ void tile_loop(const WaveSlot<G> &ws, int64_t gw, int64_t nw, int64_t M, const float *X,
                                          int nin, const float *ret, const float *V, const float *act,
                                          const float *lp_old, Body &&body, bool first_issued = false) {
  const int64_t ntiles = uniform_i64((M + 31) / 32), nfull = uniform_i64(M / 32);
  constexpr bool FIXED = G::NIC == NIN_CONT;  // the 13-input heads: the f32 path's slot loaders
  auto prefetch = [&](float *slot, int64_t row0) {
    prefetch_any<KIND, G>(ws, slot, row0, X, nin, ret, V, act, lp_old, M);
  };
  int cb = 0;
  MHPPO_MARK(0);
  if (gw < nfull && !first_issued) prefetch(ws.inb, gw * 32);
  for (int64_t tile = gw; tile < ntiles; tile += nw, cb ^= 1) {
    const int64_t row0 = tile * 32;
    const int nrows = (int)min((int64_t)32, M - row0);
    float *slot = ws.inb + cb * G::IN_SZ;
    const int64_t nxt = tile + nw;
    if (nxt < nfull) {
      prefetch(ws.inb + (cb ^ 1) * G::IN_SZ, nxt * 32);
      if constexpr (FIXED) wait_vmcnt<prefetch_ops<KIND>()>();
      else wait_vmcnt<prefetch_g_ops<KIND, G>()>();
    } else if (tile < nfull) {
      wait_vmcnt<0>();
    } else {
      if constexpr (FIXED) load_tile_sync<KIND, LY>(slot, X, NIN_CONT, ret, V, act, lp_old, row0, nrows, ws.l);
      else load_sync_g<KIND, G>(slot, X, nin, ret, V, act, lp_old, row0, nrows, ws.l);
    }
    wave_sync();  // the tile's inputs have landed
    MHPPO_MARK(1);  // timing builds: the tile-input wait
    body(slot, row0, nrows);
  }
  MHPPO_MARK_FLUSH();
}
// The four waves' gradient partials folded per block through LDS (fixed order, float64): one
// float64 partial per block, a quarter of the per-wave partials' bytes for the two-stage
// reduction to write and read.  The weight images and tile slots are dead once every wave has
// left its tile loop (the first barrier); the second publishes the four partials.
template <class G, class PassT>
__device__ __forceinline__ void fold_partials(PassT &p, const WaveSlot<G> &ws, char *L8, int w, int tid, int np,
                                              double *__restrict__ gblk, double *__restrict__ dblk) {
  static_assert(WAVES * Packed(G::K1 - 1, G::NOUT).NP * 4 + 8 + WAVES * 3 * 8 <= G::LDS_BYTES,
                "the four partials fit the kernel's LDS");
  __syncthreads();
  float *part = reinterpret_cast<float *>(L8);
  double *dl = reinterpret_cast<double *>(L8 + (WAVES * np * 4 + 7) / 8 * 8);
  p.finish(ws, part + w * np, dl + w * 3);
  __syncthreads();
  for (int k = tid; k < np; k += 64 * WAVES)
    gblk[k] = (((double)part[k] + (double)part[np + k]) + (double)part[2 * np + k]) + (double)part[3 * np + k];
  if (tid < 3) dblk[tid] = ((dl[tid] + dl[3 + tid]) + dl[6 + tid]) + dl[9 + tid];
}
}  // namespace x3

// the configuration of a single-net pass: the 13-input geometry runs hand-placed, every other
// geometry is a choice head's net
template <int KIND, class G>
using pass_cfg = std::conditional_t<
    G::NIC == NIN_CONT, std::conditional_t<KIND == K_CRITIC, x3::cfg::Critic13, x3::cfg::Actor13>,
    std::conditional_t<KIND == K_CRITIC, x3::cfg::ChoiceCritic, x3::cfg::ChoiceActor>>;

template <int KIND, class G>
__global__ void __launch_bounds__(64 * x3::WAVES)
    k_mlp_train_x3(const float *__restrict__ W, const float *__restrict__ X, int nin, int64_t M,
                   const float *__restrict__ ret, float *__restrict__ V, const float *__restrict__ act,
                   const float *__restrict__ lp_old, const double *__restrict__ stats,
                   const double *__restrict__ counts, double m_global, float out_mean, float out_std,
                   double *__restrict__ gpart, double *__restrict__ dpart) {
  using namespace x3;
  extern __shared__ float lds[];
  char *L8 = reinterpret_cast<char *>(lds);
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const WaveSlot<G> ws(L8 + G::NET_B, w, l);
  const int64_t gw = (int64_t)blockIdx.x * WAVES + w, nw = (int64_t)gridDim.x * WAVES;
  prefetch_first<KIND, G>(ws, gw, M, X, nin, ret, V, act, lp_old);
  stage_net<G>(W, L8, tid, nin);
  __syncthreads();
  static_assert((KIND == K_CONT) == (KIND != K_CRITIC && G::NIC == NIN_CONT), "the continuous actor has 13 inputs");
  Pass<KIND, G, pass_cfg<KIND, G>> p;
  p.init(L8, ws, nin, counts, m_global);
  float meanf = 0.f, stdf = 1.f;
  if (KIND != K_CRITIC) adv_norm(stats, m_global, meanf, stdf);
  const double inv_m = uniform_d(1.0 / m_global);
  tile_loop<KIND, G>(
      ws, gw, nw, M, X, nin, ret, V, act, lp_old,
      [&](const float *slot, int64_t row0, int nrows) {
        p.tile(ws, slot, row0, nrows, V, meanf, stdf, inv_m, out_mean, out_std);
      },
      true);
  p.drain();
  const int np = Packed(geo_nin<G>(nin), G::NOUT).NP;
  fold_partials<G>(p, ws, L8, w, tid, np, gpart + (size_t)blockIdx.x * np, dpart + blockIdx.x * 3);
}

// Actor pass of epoch e fused with the critic pass of epoch e + 1 (Algo_PPO.train_model_c
// :778-815 run as a pipeline: the actor of epoch e needs only V_e and the advantage sums of the
// critic pass e; the critic of epoch e + 1 needs only the critic's Adam step e).  Both nets
// train on the same tile: one input load, one launch and one weight-staging prologue instead of
// two.  The actor reads V_e from the tile's prefetched inputs before the critic overwrites those
// rows of V with V_{e+1} (each tile belongs to one wave; its inputs land one tile ahead).
// Partials: actor at gpart[gw], critic at gpart[nw + gw] (and dpart likewise).
__global__ void __launch_bounds__(64 * x3::WAVES)
    k_mlp_train_x3_pair(const float *__restrict__ Wa, const float *__restrict__ Wc, const float *__restrict__ X,
                        int64_t M, const float *__restrict__ ret, float *__restrict__ V,
                        const float *__restrict__ act, const float *__restrict__ lp_old,
                        const double *__restrict__ stats, double m_global, float out_mean, float out_std,
                        double *__restrict__ gpart, double *__restrict__ dpart) {
  using namespace x3;
  extern __shared__ float lds[];
  char *L8 = reinterpret_cast<char *>(lds);
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  using G = G13;
  const WaveSlot<G> ws(L8 + 2 * G::NET_B, w, l);
  const int64_t gw = (int64_t)blockIdx.x * WAVES + w, nw = (int64_t)gridDim.x * WAVES;
  prefetch_first<K_CONT, G>(ws, gw, M, X, NIN_CONT, ret, V, act, lp_old);
  stage_net<G>(Wa, L8, tid, NIN_CONT);
  stage_net<G>(Wc, L8 + G::NET_B, tid, NIN_CONT);
  __syncthreads();
  Pass<K_CONT, G, cfg::Pair13> pa;
  Pass<K_CRITIC, G, cfg::Pair13> pc;
  pa.init(L8, ws);
  pc.init(L8 + G::NET_B, ws);
  float meanf, stdf;
  adv_norm(stats, m_global, meanf, stdf);
  const double inv_m = uniform_d(1.0 / m_global);
  tile_loop<K_CONT, G>(
      ws, gw, nw, M, X, NIN_CONT, ret, V, act, lp_old,
      [&](const float *slot, int64_t row0, int nrows) {
        pa.tile(ws, slot, row0, nrows, V, meanf, stdf, inv_m, out_mean, out_std);
        pc.tile(ws, slot, row0, nrows, V, 0.f, 1.f, inv_m, out_mean, out_std);
      },
      true);
  constexpr int NWP = Packed(NIN_CONT, 1).NP;
  const int64_t nb = gridDim.x, b = blockIdx.x;
  fold_partials<G>(pa, ws, L8, w, tid, NWP, gpart + (size_t)b * NWP, dpart + b * 3);
  fold_partials<G>(pc, ws, L8, w, tid, NWP, gpart + (size_t)(nb + b) * NWP, dpart + (nb + b) * 3);
}
}  // namespace
