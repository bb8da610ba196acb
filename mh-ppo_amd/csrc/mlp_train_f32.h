// mlp_train_f32.h — the exact-f32 train kernel k_mlp_train<KIND, KS, PF> and its launcher: fused
// forward + loss gradient + backward + weight gradient of one Model_PPO head (n_in -> 32 -> 64 ->
// 32 -> n_out, ReLU; Coop-MH-PPO-scalable.py:42-93) over M rows, on f32 MFMA
// (v_mfma_f32_32x32x2_f32, exact fp32 products/sums in k order).  It is the reference the
// split-precision kernel (mlp_x3.h) is tested against, the kernel behind MHPPO_TRAIN_EXACT_F32,
// and the default for choice heads wider than the split kernel takes (n_in > 54).
// Replaces, per epoch and head, the torch forward GEMMs, autograd backward and the
// K = M weight-gradient GEMMs of train_model_c / train_model_d (:778-851).
//
// Geometry: one wave owns a 32-row tile at a time (grid-stride over tiles) and keeps
// its running weight gradient in registers; the waves of a block share the weights
// staged in LDS (padded strides, conflict-free operand reads).
// Orientation (both kernel families): activations are held TRANSPOSED, H^T [features x 32 rows]:
// the MFMA C tile has the row on the lane (l & 31) and the features in the 16 registers
// (feature(r, l) = (r&3) + 8(r>>2) + 4(l>>5)), so register s of a layer's output is the
// B operand of k-step s of the next layer (k order feature(s, l), matched by the
// A-operand weight reads) — no data movement between layers, forward or backward.
// Weight gradients sum over rows, i.e. need rows on the K axis: the delta and
// activation tiles go through a wave-local LDS transpose [feature][row] (stride 33) for
// those MFMAs; bias gradients are row sums of the same LDS tiles.
//
// Kinds (the loss the head is trained on; both kernel families):
//   K_CRITIC  V = net(x); writes V, accumulates (sum A, sum A^2) of A = G - V (the
//             advantage statistics, :786-787 / :825-826) and the MSE loss; dV = 2(V-G)/M.
//   K_CONT    continuous actor: mu = tanh(y)*std + mean; A normalised from the GLOBAL
//             statistics; MVN log-prob, float64 ratio, clip surrogate (:795-806);
//             dy = dL/dmu * std * (1 - tanh^2).
//   K_CHOICE  choice actor: p = softmax(y0, y1); the reference's M x M Categorical
//             broadcast (:828-842) in its exact O(M) form: each row contributes
//             sum_k counts[k] * f(r_k, A) with r_k = p_k / exp(logp_old); dL/dp through the
//             pn = p / sum(p) normalisation and the clamp, then the softmax Jacobian.
// The per-row arithmetic of the three kinds is ppo_heads.h's (one copy, with host tests); the few
// places where a call would change a train kernel's instruction text restate it and say so.
// The 13-input heads (PF: critic / continuous actor) run 8 waves per block (2 per SIMD, <= 256
// VGPRs) with the next tile's inputs prefetched into a double-buffered LDS slot by LDS-DMA; the
// other instantiations (choice obs of up to 64 features) run 4 waves and load the next tile
// through registers; their dW1 is one 32x32 tile per 32 input columns.
// Outputs per wave: the packed torch-layout gradient (float) and three float64 partial sums;
// k_grad_stage1 / k_grad_stage2 (mlp_grad_reduce.h) sum the per-wave partials in fixed order.
// Part of the mlp_train.hip translation unit (one anonymous namespace); not for inclusion elsewhere.
#pragma once
#include <math.h>

#include "mlp_tile.h"
#include "ppo_heads.h"    // the heads' per-row arithmetic; surr_and_grad (ppo_math.h)
#include "rollout_dev.h"  // MHPPO_MARK

using namespace mhppo;

namespace {
__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
// scheduling fence between phases: keeps the scheduler from hoisting the next phase's LDS
// operand reads (and their registers) into the current one
__device__ __forceinline__ void phase() { __builtin_amdgcn_sched_barrier(0); }
__device__ __forceinline__ float relu0(float x) { return __builtin_fmaxf(x, 0.0f); }
// v[r] = relu(v[r] + b[feature(r, l)]): the 4 features of register group q are contiguous
__device__ __forceinline__ void bias_relu(f32x16 &v, const float *b, int kh) {
  const float4 *b4 = reinterpret_cast<const float4 *>(b);
#pragma unroll
  for (int q = 0; q < 4; q++) {
    float4 c = b4[2 * q + kh];
    v[4 * q + 0] = relu0(v[4 * q + 0] + c.x);
    v[4 * q + 1] = relu0(v[4 * q + 1] + c.y);
    v[4 * q + 2] = relu0(v[4 * q + 2] + c.z);
    v[4 * q + 3] = relu0(v[4 * q + 3] + c.w);
  }
}
// sum_r w[feature(r, l)] * h[r] over this lane's 16 features
__device__ __forceinline__ float dot16(const float *w, const f32x16 &h, int kh) {
  float part = 0.0f;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    float4 c = reinterpret_cast<const float4 *>(w)[2 * q + kh];
    part = fmaf(c.x, h[4 * q], part);
    part = fmaf(c.y, h[4 * q + 1], part);
    part = fmaf(c.z, h[4 * q + 2], part);
    part = fmaf(c.w, h[4 * q + 3], part);
  }
  return part;
}
// store a C tile (lane = row j, registers = feature(r,l)) as T[feature][row]
__device__ __forceinline__ void put_tile(float *T, const f32x16 &v, int l) {
#pragma unroll
  for (int r = 0; r < 16; r++) T[feat(r, l) * ST + (l & 31)] = v[r];
}
// row sum of T[f][0..31] for f = l & 31 (lanes >= 32 return the same sum)
__device__ __forceinline__ float row_sum(const float *T, int l) {
  const float *p = T + (l & 31) * ST;
  float s = 0.0f;
#pragma unroll
  for (int c = 0; c < 32; c++) s += p[c];
  return s;
}

template <int KIND, int KS, bool PF>
__global__ void __launch_bounds__(PF ? 512 : 256)  // 64 * Lay::WAVES
    k_mlp_train(const float *__restrict__ W, const float *__restrict__ X, int nin, int64_t M,
                const float *__restrict__ ret, float *__restrict__ V, const float *__restrict__ act,
                const float *__restrict__ lp_old, const double *__restrict__ stats,
                const double *__restrict__ counts, double m_global, float out_mean, float out_std,
                float *__restrict__ gpart, double *__restrict__ dpart) {
  constexpr int NOUT = KIND == K_CHOICE ? 2 : 1;
  using LY = Lay<KS, PF, NOUT>;
  // 13-input heads: 13 < 2 KS = 14, so layer 1 has a free input column for the bias
  constexpr bool FOLD_B1 = PF;
  constexpr int WAVES = LY::WAVES;
  extern __shared__ float lds[];
  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: tile bookkeeping in SGPRs
  if (PF) nin = NIN_CONT;
  // packed torch-layout offsets
  const int G_W1 = 0, G_B1 = 32 * nin, G_W2 = G_B1 + 32, G_B2 = G_W2 + 64 * 32, G_W3 = G_B2 + 64,
            G_B3 = G_W3 + 32 * 64, G_W4 = G_B3 + 32, G_B4 = G_W4 + 32 * NOUT, NWP = G_B4 + NOUT;
  // ---- stage weights (padded strides, zero padding).  Every global load is issued before
  // the first LDS store (one memory round trip; a strided load -> store loop per array costs
  // one dependent trip per iteration, ~24 per launch).
  {
    constexpr int NT = 64 * WAVES, N1 = (32 * LY::S1 + NT - 1) / NT, N2 = 2048 / NT;
    static_assert(2048 % NT == 0 && NT >= 64, "staging: block size");
    float v1[N1], v2[N2], v3[N2];
#pragma unroll
    for (int q = 0; q < N1; q++) {
      const int i = tid + q * NT, r = i / LY::S1, c = i % LY::S1;
      // FOLD_B1: b1 rides in the padding column nin of W1 against a constant-1 input
      v1[q] = i >= 32 * LY::S1 ? 0.0f
                               : (c < nin ? W[G_W1 + r * nin + c] : ((FOLD_B1 && c == nin) ? W[G_B1 + r] : 0.0f));
    }
#pragma unroll
    for (int q = 0; q < N2; q++) {
      v2[q] = W[G_W2 + tid + q * NT];
      v3[q] = W[G_W3 + tid + q * NT];
    }
    const float vb1 = tid < 32 ? W[G_B1 + tid] : 0.0f, vb3 = tid < 32 ? W[G_B3 + tid] : 0.0f;
    const float vb2 = tid < 64 ? W[G_B2 + tid] : 0.0f, vw4 = tid < 32 * NOUT ? W[G_W4 + tid] : 0.0f;
    const float vb4 = tid < NOUT ? W[G_B4 + tid] : 0.0f;
#pragma unroll
    for (int q = 0; q < N1; q++) {
      const int i = tid + q * NT;
      if (i < 32 * LY::S1) lds[LY::O_W1 + i] = v1[q];
    }
#pragma unroll
    for (int q = 0; q < N2; q++) {
      const int i = tid + q * NT;
      lds[LY::O_W2 + (i >> 5) * S2 + (i & 31)] = v2[q];
      lds[LY::O_W3 + (i >> 6) * S3 + (i & 63)] = v3[q];
    }
    if (tid < 32) {
      lds[LY::O_B1 + tid] = vb1;
      lds[LY::O_B3 + tid] = vb3;
    }
    if (tid < 64) lds[LY::O_B2 + tid] = vb2;
    if (tid < 32 * NOUT) lds[LY::O_W4 + tid] = vw4;
    if (tid < NOUT) lds[LY::O_B4 + tid] = vb4;
  }
  __syncthreads();
  float *ws = lds + LY::O_WEND + w * LY::WAVE_LDS;
  float *T0 = ws + LY::O_T, *T1 = T0 + TILE, *T2 = T1 + TILE;
  const float b40 = lds[LY::O_B4], b41 = NOUT == 2 ? lds[LY::O_B4 + 1] : 0.0f;
  const int j = l & 31;
  const int kh = l >> 5;

  // persistent accumulators (gW1b: input columns 32..63 of dW1, heads with n_in > 32)
  constexpr bool W1B = !PF && 2 * KS > 32;
  f32x16 gW1 = zero16(), gW1b = zero16(), gW2a = zero16(), gW2b = zero16(), gW3a = zero16(), gW3b = zero16();
  // 13-input heads: dW1 = dH1^T X is [32 features x 14 columns] — two 16x16 tiles of the
  // 16x16x4 MFMA (half the cycles of one 32x32 tile); D row (l>>4)*4 + r, column l & 15
  f32x4 gW1q[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  float gB1 = 0.f, gB2 = 0.f, gB3 = 0.f, gW40 = 0.f, gW41 = 0.f, gB40 = 0.f, gB41 = 0.f;
  // float64 running sums (loss, sum A, sum A^2) live in LDS, one slot per lane of the low
  // half-wave: keeping them in VGPRs spills, and a spill reload's vmcnt(0) drains the prefetch
  double *dacc = reinterpret_cast<double *>(lds + LY::O_DACC) + w * 96 + j;
  if (kh == 0) dacc[0] = dacc[32] = dacc[64] = 0.0;
  float meanf = 0.f, stdf = 1.f;
  if (KIND != K_CRITIC) {  // ppo_heads.h adv_moments, restated (stats[1] is loaded after the mean's division)
    double mean = stats[0] / m_global;
    double var = (stats[1] - stats[0] * mean) / (m_global - 1.0);
    meanf = (float)mean;
    stdf = (float)sqrt(var > 0 ? var : 0.0);
  }
  const double inv_m = 1.0 / m_global;
  const int64_t ntiles = (M + 31) / 32, nfull = PF ? M / 32 : 0;
  const int64_t gw = (int64_t)blockIdx.x * WAVES + w, nw = (int64_t)gridDim.x * WAVES;

  int cb = 0;
  MHPPO_MARK(0);
  if (PF && gw < nfull) prefetch_tile<KIND, LY>(ws + LY::O_IN, X, ret, V, act, lp_old, gw * 32, l, M);
  TileRegs<LY> tnext;  // non-PF: the next tile's inputs in registers
  if (!PF && gw < ntiles)
    load_tile_regs<KIND, LY>(tnext, X, nin, ret, V, act, lp_old, gw * 32, (int)min((int64_t)32, M - gw * 32), l);
  for (int64_t tile = gw; tile < ntiles; tile += nw, cb ^= (PF ? 1 : 0)) {
    const int64_t row0 = tile * 32;
    const int nrows = (int)min((int64_t)32, M - row0);
    float *slot = ws + LY::O_IN + cb * LY::IN_SZ;
    if constexpr (PF) {
      const int64_t nxt = tile + nw;
      if (nxt < nfull) {
        prefetch_tile<KIND, LY>(ws + LY::O_IN + (cb ^ 1) * LY::IN_SZ, X, ret, V, act, lp_old, nxt * 32, l, M);
        wait_vmcnt<prefetch_ops<KIND>()>();  // this tile's DMA (issued one iteration earlier) has landed
      } else if (tile < nfull) {
        wait_vmcnt<0>();
      } else {
        load_tile_sync<KIND, LY>(slot, X, nin, ret, V, act, lp_old, row0, nrows, l);
      }
    } else {
      // this tile's inputs were loaded into registers one iteration earlier (the first tile's
      // before the loop); the next tile's loads are in flight during this tile's compute
      store_tile_regs<KIND, LY>(slot, tnext, nin, l);
      const int64_t nt = tile + nw;
      if (nt < ntiles)
        load_tile_regs<KIND, LY>(tnext, X, nin, ret, V, act, lp_old, nt * 32, (int)min((int64_t)32, M - nt * 32), l);
    }
    wave_sync();
    MHPPO_MARK(1);  // tile inputs landed
    const float *Xs = slot + LY::IN_X;
    // ---- forward
    f32x16 h1 = zero16();
#pragma unroll
    for (int s = 0; s < KS; s++) {
      int k = 2 * s + kh;
      float a = lds[LY::O_W1 + j * LY::S1 + k];
      float b = (k < nin) ? Xs[j * nin + k] : ((FOLD_B1 && k == nin) ? 1.0f : 0.0f);
      h1 = mfma(a, b, h1);
    }
    if constexpr (FOLD_B1) {  // the last fmaf of the chain added b1 (fma(b, 1, acc) == acc + b)
#pragma unroll
      for (int r = 0; r < 16; r++) h1[r] = relu0(h1[r]);
    } else {
      bias_relu(h1, lds + LY::O_B1, kh);
    }
    phase();
    f32x16 h2a = zero16(), h2b = zero16();
#pragma unroll
    for (int s = 0; s < 16; s++) {
      int k = feat(s, l);
      h2a = mfma(lds[LY::O_W2 + j * S2 + k], h1[s], h2a);
      h2b = mfma(lds[LY::O_W2 + (32 + j) * S2 + k], h1[s], h2b);
    }
    bias_relu(h2a, lds + LY::O_B2, kh);
    bias_relu(h2b, lds + LY::O_B2 + 32, kh);
    phase();
    f32x16 h3 = zero16();
#pragma unroll
    for (int s = 0; s < 16; s++) h3 = mfma(lds[LY::O_W3 + j * S3 + feat(s, l)], h2a[s], h3);
#pragma unroll
    for (int s = 0; s < 16; s++) h3 = mfma(lds[LY::O_W3 + j * S3 + 32 + feat(s, l)], h2b[s], h3);
    // h2 leaves the registers: ReLU masks as bits, h2b parked in T2 for dW3b, h2a stays
    // live only until the dW4/dB3 row sums have freed T0
    uint32_t m2 = 0;
#pragma unroll
    for (int r = 0; r < 16; r++) m2 |= ((h2a[r] > 0.0f) ? 1u : 0u) << r | ((h2b[r] > 0.0f) ? 1u : 0u) << (16 + r);
    put_tile(T2, h2b, l);
    bias_relu(h3, lds + LY::O_B3, kh);
    float part0 = dot16(lds + LY::O_W4, h3, kh);
    const float y0 = (part0 + __shfl_xor(part0, 32)) + b40;
    float y1 = 0.0f;
    if constexpr (NOUT == 2) {
      float part1 = dot16(lds + LY::O_W4 + 32, h3, kh);
      y1 = (part1 + __shfl_xor(part1, 32)) + b41;
    }
    MHPPO_MARK(2);  // forward
    // ---- loss gradient dL/dy for this lane's row
    const bool valid = j < nrows;
    float dy0 = 0.0f, dy1 = 0.0f;
    if (valid) {
      const float rt = slot[LY::IN_S0 + j];
      if constexpr (KIND == K_CRITIC) {
        const float v = y0;
        // the store's range is the tile's rows in the batch: no lane can write past the batch
        if (kh == 0) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsrc(V + row0, 4 * nrows), 4 * j, 0, 0);
        const float a = rt - v;
        const float d = v - rt;
        if (kh == 0) {
          dacc[0] += (double)d * (double)d;
          dacc[32] += (double)a;
          dacc[64] += (double)a * (double)a;
        }
        dy0 = (float)(2.0 * inv_m * (double)d);
      } else if constexpr (KIND == K_CONT) {
        float t, x;
        const float mu = finish_cont<LibmUpdate>(y0, out_mean, out_std, t);
        const float A = adv_normalised(rt - slot[LY::IN_S0 + 32 + j], meanf, stdf);
        const float lp = cont_logp_x(slot[LY::IN_S1 + j], mu, x);
        const double r = exp((double)lp - (double)slot[LY::IN_S1 + 32 + j]);
        double dfdr;
        const double f = surr_and_grad(r, (double)A, dfdr);
        if (kh == 0) dacc[0] += f;
        const float dmu = cont_dmu(inv_m, dfdr, r, x);
        dy0 = (dmu * out_std) * (1.0f - t * t);
      } else {
        // This branch restates ppo_heads.h softmax_pair, cat_normalise, choice_term, cat_grad_p and
        // softmax_jacobian (calls compile to other code in the n_in > 32 instantiations).
        // softmax over the pair (as torch: shift by the max), pn = p / (p0 + p1)
        const float mx = fmaxf(y0, y1);
        const float e0 = expf(y0 - mx), e1 = expf(y1 - mx);
        const float se = e0 + e1;
        const float p[2] = {e0 / se, e1 / se};
        const float A = adv_normalised(rt - slot[LY::IN_S0 + 32 + j], meanf, stdf);
        const double old = (double)slot[LY::IN_S1 + j];
        const float sp = p[0] + p[1];
        const float pn[2] = {p[0] / sp, p[1] / sp};
        const float eps = CAT_EPS, hi = CAT_HI;
        const double inv_m2 = inv_m * inv_m;
        // reference: every row meets every action with the global counts (the M x M
        // broadcast); per-row mode (counts == NULL, opt-in bug fix): the row's own action
        // with weight M_global, i.e. the standard mean over rows of the PPO surrogate
        const int a_row = counts ? 0 : (int)slot[LY::IN_S1 + 32 + j];
        double dlp[2], f = 0.0;
#pragma unroll
        for (int k = 0; k < 2; k++) {
          const double w = counts ? counts[k] : (k == a_row ? m_global : 0.0);
          const float pc = pn[k] < eps ? eps : (pn[k] > hi ? hi : pn[k]);
          const double r = exp((double)logf(pc) - old);
          double dfdr;
          const double fk = surr_and_grad(r, (double)A, dfdr);
          if (w != 0.0) f += w * fk;  // weight 0 (per-row: the other action) is no term: 0 * inf stays out
          const double pass = (pn[k] >= eps && pn[k] <= hi) ? 1.0 : 0.0;
          dlp[k] = inv_m2 * w * dfdr * r * pass / (double)pc;  // dL/dpn_k
        }
        if (kh == 0) dacc[0] += f;
        const double sd = (double)sp;
        const double g0 = (dlp[0] * (1.0 - pn[0]) - dlp[1] * pn[1]) / sd;  // dL/dp_k
        const double g1 = (dlp[1] * (1.0 - pn[1]) - dlp[0] * pn[0]) / sd;
        const double dot = (double)p[0] * g0 + (double)p[1] * g1;
        dy0 = (float)((double)p[0] * (g0 - dot));  // softmax Jacobian
        dy1 = (float)((double)p[1] * (g1 - dot));
      }
    }
    MHPPO_MARK(3);  // loss gradient
    gB40 += (kh == 0) ? dy0 : 0.0f;
    gB41 += (kh == 0) ? dy1 : 0.0f;
    // ---- layer 4 backward: dW4 = rowsum(dy * h3), dH3 = W4^T dy masked
    f32x16 g = zero16(), g1v = zero16();
#pragma unroll
    for (int q = 0; q < 4; q++) {
      float4 c = reinterpret_cast<const float4 *>(lds + LY::O_W4)[2 * q + kh];
      float cw[4] = {c.x, c.y, c.z, c.w};
      float cw1[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (NOUT == 2) {
        float4 c1 = reinterpret_cast<const float4 *>(lds + LY::O_W4 + 32)[2 * q + kh];
        cw1[0] = c1.x, cw1[1] = c1.y, cw1[2] = c1.z, cw1[3] = c1.w;
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int r = 4 * q + i;
        g[r] = dy0 * h3[r];
        if constexpr (NOUT == 2) {
          g1v[r] = dy1 * h3[r];
          h3[r] = (h3[r] > 0.0f) ? fmaf(cw1[i], dy1, cw[i] * dy0) : 0.0f;  // h3 := dH3^T
        } else {
          h3[r] = (h3[r] > 0.0f) ? cw[i] * dy0 : 0.0f;
        }
      }
    }
    put_tile(T0, g, l);
    put_tile(T1, h3, l);
    wave_sync();
    phase();
    if (kh == 0) {
      gW40 += row_sum(T0, l);
      gB3 += row_sum(T1, l);
    }
    if constexpr (NOUT == 2) {
      wave_sync();
      put_tile(T0, g1v, l);
      wave_sync();
      if (kh == 0) gW41 += row_sum(T0, l);
    }
    wave_sync();
    phase();
    put_tile(T0, h2a, l);
    wave_sync();
    phase();
    // dW3[:, 0:32] += dH3^T . H2a ; dW3[:, 32:64] += dH3^T . H2b
#pragma unroll
    for (int s = 0; s < 16; s++) {
      int k = 2 * s + kh;
      gW3a = mfma(T1[j * ST + k], T0[j * ST + k], gW3a);
    }
#pragma unroll
    for (int s = 0; s < 16; s++) {
      int k = 2 * s + kh;
      gW3b = mfma(T1[j * ST + k], T2[j * ST + k], gW3b);
    }
    // dH2^T = W3^T . dH3^T, masked by h2 > 0
    f32x16 d2a = zero16(), d2b = zero16();
#pragma unroll
    for (int s = 0; s < 16; s++) {
      int f = feat(s, l);
      d2a = mfma(lds[LY::O_W3 + f * S3 + j], h3[s], d2a);
      d2b = mfma(lds[LY::O_W3 + f * S3 + 32 + j], h3[s], d2b);
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
      d2a[r] = ((m2 >> r) & 1u) ? d2a[r] : 0.0f;
      d2b[r] = ((m2 >> (16 + r)) & 1u) ? d2b[r] : 0.0f;
    }
    MHPPO_MARK(4);  // layer-4 backward, dW3 + dH2
    wave_sync();
    phase();
    put_tile(T0, d2a, l);
    put_tile(T1, d2b, l);
    put_tile(T2, h1, l);
    wave_sync();
    phase();
    gB2 += row_sum(kh ? T1 : T0, l);
    // dW2 += dH2^T . H1
#pragma unroll
    for (int s = 0; s < 16; s++) {
      int k = 2 * s + kh;
      float b = T2[j * ST + k];
      gW2a = mfma(T0[j * ST + k], b, gW2a);
      gW2b = mfma(T1[j * ST + k], b, gW2b);
    }
    // dH1^T = W2^T . dH2^T, masked by h1 > 0
    f32x16 d1 = zero16();
#pragma unroll
    for (int s = 0; s < 16; s++) d1 = mfma(lds[LY::O_W2 + feat(s, l) * S2 + j], d2a[s], d1);
#pragma unroll
    for (int s = 0; s < 16; s++) d1 = mfma(lds[LY::O_W2 + (32 + feat(s, l)) * S2 + j], d2b[s], d1);
#pragma unroll
    for (int r = 0; r < 16; r++) d1[r] = (h1[r] > 0.0f) ? d1[r] : 0.0f;
    MHPPO_MARK(5);  // dW2 + dH1
    wave_sync();
    phase();
    put_tile(T0, d1, l);
    wave_sync();
    phase();
    if (!FOLD_B1 && kh == 0) gB1 += row_sum(T0, l);  // FOLD_B1: column nin of dW1 is dB1
    // dW1 += dH1^T . X
    if constexpr (PF) {  // rows 4s..4s+3 per step, ascending: the same fmaf chain order
#pragma unroll
      for (int s = 0; s < 8; s++) {
        const int rr = 4 * s + (l >> 4), jj = l & 15;
        const float b = (jj < nin) ? Xs[rr * nin + jj] : ((FOLD_B1 && jj == nin) ? 1.0f : 0.0f);
#pragma unroll
        for (int ft = 0; ft < 2; ft++) gW1q[ft] = mfma16(T0[(16 * ft + (l & 15)) * ST + rr], b, gW1q[ft]);
      }
    } else {
#pragma unroll
      for (int s = 0; s < 16; s++) {
        int k = 2 * s + kh;
        float b = (j < nin) ? Xs[k * nin + j] : ((FOLD_B1 && j == nin) ? 1.0f : 0.0f);
        gW1 = mfma(T0[j * ST + k], b, gW1);
      }
      if constexpr (W1B) {
#pragma unroll
        for (int s = 0; s < 16; s++) {
          int k = 2 * s + kh;
          float b = (32 + j < nin) ? Xs[k * nin + 32 + j] : 0.0f;
          gW1b = mfma(T0[j * ST + k], b, gW1b);
        }
      }
    }
    wave_sync();
    phase();
    MHPPO_MARK(6);  // dW1 (timing builds only)
  }
  MHPPO_MARK_FLUSH();
  // ---- write this wave's partial gradient (packed torch layout)
  float *gp = gpart + (size_t)gw * NWP;
#pragma unroll
  for (int r = 0; r < 16; r++) {
    int f = feat(r, l);
    if (!PF && j < nin) gp[G_W1 + f * nin + j] = gW1[r];
    if (W1B && 32 + j < nin) gp[G_W1 + f * nin + 32 + j] = gW1b[r];
    gp[G_W2 + f * 32 + j] = gW2a[r];
    gp[G_W2 + (32 + f) * 32 + j] = gW2b[r];
    gp[G_W3 + f * 64 + j] = gW3a[r];
    gp[G_W3 + f * 64 + 32 + j] = gW3b[r];
  }
  if constexpr (PF) {
#pragma unroll
    for (int ft = 0; ft < 2; ft++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int f = 16 * ft + (l >> 4) * 4 + r, jj = l & 15;
        if (jj < nin) gp[G_W1 + f * nin + jj] = gW1q[ft][r];
        if (FOLD_B1 && jj == nin) gp[G_B1 + f] = gW1q[ft][r];
      }
  }
  if (kh == 0) {
    if (!FOLD_B1) gp[G_B1 + j] = gB1;
    gp[G_B3 + j] = gB3;
    gp[G_W4 + j] = gW40;
    if (NOUT == 2) gp[G_W4 + 32 + j] = gW41;
  }
  gp[G_B2 + l] = gB2;  // lanes 0-31: features 0-31 (T0), lanes 32-63: 32-63 (T1)
  // b4 and float64 sums: wave reductions
  float b4s0 = gB40, b4s1 = gB41;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    b4s0 += __shfl_xor(b4s0, o);
    b4s1 += __shfl_xor(b4s1, o);
  }
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  if (kh == 0) s0 = dacc[0], s1 = dacc[32], s2 = dacc[64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s0 += __shfl_xor(s0, o);
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if (l == 0) {
    gp[G_B4] = b4s0;
    if (NOUT == 2) gp[G_B4 + 1] = b4s1;
    dpart[gw * 3 + 0] = s0;
    dpart[gw * 3 + 1] = s1;
    dpart[gw * 3 + 2] = s2;
  }
}

template <int KIND, int KS, bool PF>
void launch(dim3 grid, hipStream_t s, const float *packed, const float *X, int nin, int64_t M, const float *ret,
            float *value, const float *act, const float *logp_old, const double *stats, const double *counts,
            double m_global, float out_mean, float out_std, float *gp, double *dp) {
  using LY = Lay<KS, PF, (KIND == K_CHOICE ? 2 : 1)>;
  hipLaunchKernelGGL((k_mlp_train<KIND, KS, PF>), grid, dim3(64 * LY::WAVES), sizeof(float) * LY::FLOATS, s,
                     packed, X, nin, M, ret, value, act, logp_old, stats, counts, m_global, out_mean, out_std, gp, dp);
}
}  // namespace
