// rollout_policy.h — the rollout's policy step, one row per (env, slot, ped): the obs_car_ped
// features and the cross / wait actor picked by action_d.
//   rec_map / rec_index / feat_row   where a row's features are recorded (identity or compact layout)
//   namespace pol                    both actors' LDS image and one 32-row tile on f32 MFMA
//                                    (the tile primitives are mfma_tile.h's)
//   k_policy_mfma                    the shipped kernel: head-sorted 32-row tiles
//   k_policy / k_policy_sorted       the VALU bit-identity references (MHPPO_TEST_KERNELS: the test
//                                    build only)
// Part of the rollout.hip translation unit (one anonymous namespace); not for inclusion elsewhere.
#pragma once
#include "launch1d.h"
#include "ppo_heads.h"
#include "mfma_tile.h"
#include "rollout_dev.h"

namespace {
using namespace mhppo;

// Record index of segment s = env * nS + slot in the time-major records: B.rec_of[s] in the
// compact layout (-1: the segment stores no record), else s (include/mhppo.h mhppo_rollout_bufs)
// The compact layout is the scalable env's only (the variant whose car slots can be absent;
// mhppo_rollout_begin rejects rec_of for the others), so the other variants compile without it.
template <int V>
__device__ __forceinline__ const int32_t *rec_map(const mhppo_rollout_bufs &B) {
  return V == V_SCALABLE ? B.rec_of : nullptr;
}
template <int V>
__device__ __forceinline__ int64_t rec_index(const mhppo_rollout_bufs &B, int64_t s) {
  const int32_t *m = rec_map<V>(B);
  return m ? (int64_t)m[s] : s;
}
// feat_c row of policy row r = (env, slot, ped): with one pedestrian and the compact layout, feat_c
// is the step's record obs_c[t] and row r its segment's record (-1: none)
template <int V>
__device__ __forceinline__ int64_t feat_row(const mhppo_rollout_bufs &B, int P, int64_t r) {
  return P == 1 ? rec_index<V>(B, r) : r;
}

#ifdef MHPPO_TEST_KERNELS
// The VALU policy kernels (test build only, tests/lib/libmhppo_test.so: the bit-identity reference of
// k_policy_mfma, tests/test_rollout_gpu.py).  The shipped library runs k_policy_mfma alone.
template <int V>
__global__ void __launch_bounds__(TPB) k_policy(Cfg c, mhppo_mlp mc, mhppo_mlp mw, mhppo_rollout_bufs B) {
  extern __shared__ float lds[];
  const int sz = mlp_size(NF_C, 1);
  for (int i = threadIdx.x; i < sz; i += blockDim.x) {
    lds[i] = mc.packed[i];
    lds[sz + i] = mw.packed[i];
  }
  __syncthreads();
  const ObsLayout L = obs_layout(c);
  size_t r = (size_t)blockIdx.x * TPB + threadIdx.x;
  size_t R = (size_t)c.N * c.nS * c.P;
  if (r >= R) return;
  int p = (int)(r % c.P), i = (int)((r / c.P) % c.nS);
  size_t e = r / ((size_t)c.P * c.nS);
  const float *o = B.obs + e * L.obs_dim;
  float f[NF_C];
  float ex = obs_car_ped(o, L, i, p, f);
  const int64_t fr = feat_row<V>(B, c.P, (int64_t)r);
  if (fr >= 0) {
    float *fo = B.feat_c + fr * NF_C;
#pragma unroll
    for (int k = 0; k < NF_C; k++) fo[k] = f[k];
  }
  if (L.scalable && ex == 0.0f) return;  // `if exist:` gate of the scalable driver (:439)
  // action_d = 2*a - 1; cross head when action_d <= 0 (:440-445)
  bool wait = (2 * B.a_d[r] - 1) > 0;
  const float *W = wait ? lds + sz : lds;
  const mhppo_mlp &m = wait ? mw : mc;
  float out;
  mlp_forward<NF_C, 1>(W, NF_C, f, &out);
  B.out_c[r] = finish_cont<LibmRollout>(out, m.mean, m.std);  // Model_PPO type 1 (:87-89)
}

// Head-sorted policy step.  mhppo_rollout_begin lists the rows (env, slot, ped) of the
// cross head, then those of the wait head (B.rows, counts at [R], [R+1]; the choice is
// fixed for the episode); each wave takes 64 rows of ONE head, so the actor weights are
// wave-uniform and stream through the scalar cache as SGPR operands of the FMAs.  (With
// per-lane heads the weights come from LDS, and 64 lanes reading one weight cost the LDS
// pipe 64 words: that, not the FMAs, bounds k_policy.)  Same features, same fmaf chains:
// bit-identical to k_policy.  (Stale MT19937 blocks are regenerated once per episode, by the
// reset kernel: see k_policy_mfma.)
template <int V>
__global__ void __launch_bounds__(TPB) k_policy_sorted(Cfg c, const float *__restrict__ Wc,
                                                       const float *__restrict__ Ww, float mean_c, float std_c,
                                                       float mean_w, float std_w, mhppo_rollout_bufs B, Bufs eb) {
  const int lane = threadIdx.x & 63;
  const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (TPB / 64) + (threadIdx.x >> 6)));
  const int R = c.N * c.nS * c.P;
  const int32_t *__restrict__ rows = B.rows;
  const int nc = __builtin_amdgcn_readfirstlane(rows[R]), nw = __builtin_amdgcn_readfirstlane(rows[R + 1]);
  const int wc = (nc + 63) / 64;
  int head, k0, kend;
  if (gw < wc) {
    head = 0, k0 = gw * 64, kend = nc;
  } else {
    const int w2 = gw - wc;
    if (w2 * 64 >= nw) return;
    head = 1, k0 = nc + w2 * 64, kend = nc + nw;
  }
  const int k = k0 + lane;
  if (k >= kend) return;
  const int r = rows[k];
  const ObsLayout L = obs_layout(c);
  const int p = r % c.P, i = (r / c.P) % c.nS;
  const int e = r / (c.P * c.nS);
  const float *o = B.obs + (size_t)e * L.obs_dim;
  float f[NF_C];
  float ex = obs_car_ped(o, L, i, p, f);
  const int64_t fr = feat_row<V>(B, c.P, r);
  if (fr >= 0) {
    float *fo = B.feat_c + fr * NF_C;
#pragma unroll
    for (int q = 0; q < NF_C; q++) fo[q] = f[q];
  }
  if (L.scalable && ex == 0.0f) return;  // `if exist:` gate of the scalable driver (:439)
  const float out = mlp_forward13_rows(head ? Ww : Wc, f);
  B.out_c[r] = finish_cont<LibmRollout>(out, head ? mean_w : mean_c, head ? std_w : std_c);  // type 1 (:87-89)
}
#endif  // MHPPO_TEST_KERNELS

// ------------------------------------------------------- MFMA policy step
// k_policy_mfma: the head-sorted rows as 32-row tiles on f32 MFMA (v_mfma_f32_32x32x2_f32, the
// forward layout of mlp_train.hip: rows on the lanes, features in the 16 C registers), both
// actors' weights in LDS.  Bit-identical to mlp_forward13_rows: the f32 MFMA is a k-ordered
// fmaf chain (cdna_hip_programming.md §3), and the weight rows of layers 1-3 are staged
// permuted so that C register s of lane half kh holds neuron 2s + kh — k-step s of the next
// layer then feeds its inputs 2s, 2s + 1, i.e. every chain runs in ascending input order;
// the 32 -> 1 output is the same ascending fmaf chain over both lane halves.
#ifndef MHPPO_POLICY_BLOCKS_PER_CU
#define MHPPO_POLICY_BLOCKS_PER_CU 4  // k_policy_mfma blocks resident per CU (A/B builds override)
#endif
#ifndef MHPPO_POLICY_TPB
// k_policy_mfma block size: 4 waves share one LDS copy of the two actors (38.7 KB), four blocks per CU
// (the LDS bound) give four waves per SIMD (<= 128 VGPRs) to hide the MFMA chains' layer-to-layer
// latency.  r06: 256-thread blocks, more of them than fit at once at large N (below), against
// 512-thread blocks two per CU: cfg4 collect 10.85 -> 9.86 ms, cfg3 5.93 -> 5.80 ms
#define MHPPO_POLICY_TPB 256
#endif
constexpr int PTPB = MHPPO_POLICY_TPB;
namespace pol {
using namespace mhppo::mfma_tile;  // f32x16, mfma, zero16, bias_relu, row_of_neuron, S2, S3
constexpr int S1 = 15;  // odd LDS row stride of W1 (as S2, S3): conflict-free operand reads
constexpr int O_W1 = 0, O_B1 = O_W1 + 32 * S1, O_W2 = O_B1 + 32, O_B2 = O_W2 + 64 * S2, O_W3 = O_B2 + 64,
              O_B3 = O_W3 + 32 * S3, O_W4 = O_B3 + 32, O_B4 = O_W4 + 32, HEAD = (O_B4 + 1 + 3) / 4 * 4;
// Both 13 -> 32 -> 64 -> 32 -> 1 actors (torch-packed W) into LDS, [2][HEAD], the weight rows
// of layers 1-3 permuted (mfma_tile.h: LDS row row_of_neuron(n) of a layer holds neuron n), W1 rows
// zero-padded to S1.  Every global load of both nets is issued first (coalesced, in source
// order, none waiting on another), then the permuted LDS stores: one memory round trip per
// block (a strided load -> store loop per array costs ~20 dependent trips per net at the start
// of every policy launch).
template <int NT>
__device__ __forceinline__ void stage_both(float *L, const float *__restrict__ Wa, const float *__restrict__ Wb,
                                           int tid) {
  constexpr int NW1 = 32 * NF_C, N1 = (NW1 + NT - 1) / NT, N2 = 2048 / NT;
  static_assert(2048 % NT == 0 && NT >= 64, "stage_both: block size");
  const float *W[2] = {Wa, Wb};
  float v1[2][N1], v2[2][N2], v3[2][N2], vb1[2], vb2[2], vb3[2], vw4[2], vb4[2];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const float *w1 = W[h], *b1 = w1 + NW1, *w2 = b1 + 32, *b2 = w2 + 2048, *w3 = b2 + 64, *b3 = w3 + 2048,
                *w4 = b3 + 32, *b4 = w4 + 32;
#pragma unroll
    for (int q = 0; q < N1; q++) {
      const int x = tid + q * NT;
      v1[h][q] = x < NW1 ? w1[x] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < N2; q++) {
      v2[h][q] = w2[tid + q * NT];
      v3[h][q] = w3[tid + q * NT];
    }
    vb1[h] = tid < 32 ? b1[tid] : 0.0f;
    vb3[h] = tid < 32 ? b3[tid] : 0.0f;
    vw4[h] = tid < 32 ? w4[tid] : 0.0f;
    vb2[h] = tid < 64 ? b2[tid] : 0.0f;
    vb4[h] = tid == 0 ? b4[0] : 0.0f;
  }
#pragma unroll
  for (int h = 0; h < 2; h++) {
    float *Lh = L + h * HEAD;
#pragma unroll
    for (int q = 0; q < N1; q++) {
      const int x = tid + q * NT;
      if (x < NW1) {
        const int n = x / NF_C, k = x - n * NF_C;
        Lh[O_W1 + row_of_neuron(n) * S1 + k] = v1[h][q];
      }
    }
    if (tid < 64) Lh[O_W1 + (tid >> 1) * S1 + NF_C + (tid & 1)] = 0.0f;  // padding columns 13, 14
#pragma unroll
    for (int q = 0; q < N2; q++) {
      const int x = tid + q * NT;
      const int n2 = x >> 5, k2 = x & 31;  // W2 [64][32]
      Lh[O_W2 + ((n2 & 32) + row_of_neuron(n2 & 31)) * S2 + k2] = v2[h][q];
      const int n3 = x >> 6, k3 = x & 63;  // W3 [32][64]
      Lh[O_W3 + row_of_neuron(n3) * S3 + k3] = v3[h][q];
    }
    if (tid < 32) {
      Lh[O_B1 + row_of_neuron(tid)] = vb1[h];
      Lh[O_B3 + row_of_neuron(tid)] = vb3[h];
      Lh[O_W4 + tid] = vw4[h];
    }
    if (tid < 64) Lh[O_B2 + (tid & 32) + row_of_neuron(tid & 31)] = vb2[h];
    if (tid == 0) Lh[O_B4] = vb4[h];
  }
}
// One 32-row tile of one 13 -> 32 -> 64 -> 32 -> 1 actor (Wl: its LDS image above) on f32 MFMA:
// lane j of both halves holds row j's features f; returns the row's pre-tanh output in every
// lane — the oracle's ascending fmaf chains bit for bit (the permuted staging).
// Layers 2-4 are the chain of infer::tile_forward<1> (mlp_infer_tile.h) with this image's constant
// offsets: change the two together.  (No form of one shared function left both this kernel's
// instruction stream and the infer kernels' as they were: profiles/rollout_split/kernels.txt.)
__device__ __forceinline__ float actor_tile(const float *Wl, const float (&f)[NF_C + 1], int j, int kh) {
  f32x16 h1 = zero16();
#pragma unroll
  for (int s = 0; s < 7; s++) {
    // both lane halves hold the row's features: the lower half takes f[2s], the upper f[2s + 1]
    // (one v_permlane32_swap; a lane-select of the two is folded into an indexed load of f,
    // which puts f in scratch memory)
    const auto x = __builtin_amdgcn_permlane32_swap(__float_as_uint(f[2 * s]), __float_as_uint(f[2 * s + 1]), false, false);
    h1 = mfma(Wl[O_W1 + j * S1 + 2 * s + kh], __uint_as_float(x[0]), h1);
  }
  bias_relu(h1, Wl + O_B1, kh);
  f32x16 h2a = zero16(), h2b = zero16();
#pragma unroll
  for (int s = 0; s < 16; s++) {
    h2a = mfma(Wl[O_W2 + j * S2 + 2 * s + kh], h1[s], h2a);
    h2b = mfma(Wl[O_W2 + (32 + j) * S2 + 2 * s + kh], h1[s], h2b);
  }
  bias_relu(h2a, Wl + O_B2, kh);
  bias_relu(h2b, Wl + O_B2 + 32, kh);
  f32x16 h3 = zero16();
#pragma unroll
  for (int s = 0; s < 16; s++) h3 = mfma(Wl[O_W3 + j * S3 + 2 * s + kh], h2a[s], h3);
#pragma unroll
  for (int s = 0; s < 16; s++) h3 = mfma(Wl[O_W3 + j * S3 + 32 + 2 * s + kh], h2b[s], h3);
  bias_relu(h3, Wl + O_B3, kh);
  float y = 0.0f;
#pragma unroll
  for (int s = 0; s < 16; s++) {
    // neuron 2s sits in register s of the lower lane half, 2s + 1 in the upper: one
    // v_permlane32_swap gives every lane both (r[0] = neuron 2s, r[1] = neuron 2s + 1 of its row)
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(h3[s]), __float_as_uint(h3[s]), false, false);
    y = fmaf(Wl[O_W4 + 2 * s], __uint_as_float(r[0]), y);
    y = fmaf(Wl[O_W4 + 2 * s + 1], __uint_as_float(r[1]), y);
  }
  return y + Wl[O_B4];
}
}  // namespace pol

// Registers for five waves per SIMD (88 VGPRs; 120 without the bound): the LDS holds four blocks per
// CU, and the fifth slot lets a policy wave share a SIMD with a cfg4 env wave of the other rollout part
// (k_sample_env_r<2, 8, 8, 1>: 404 VGPRs): collect cfg4 -0.9 %, cfg3 -0.6 %, cfg2 -1.4 %
// (profiles/r06_rollout/ab_policy_vgpr.txt)
#ifndef MHPPO_POLICY_WPE
#define MHPPO_POLICY_WPE 5
#endif
template <int V>
__global__ void __launch_bounds__(PTPB) __attribute__((amdgpu_waves_per_eu(MHPPO_POLICY_WPE)))
k_policy_mfma(Cfg c, const float *__restrict__ Wc,
                                                      const float *__restrict__ Ww, float mean_c, float std_c,
                                                      float mean_w, float std_w, mhppo_rollout_bufs B, Bufs eb,
                                                      int part, int nparts) {
  using namespace pol;
  extern __shared__ float lds[];  // [2][HEAD]: cross, wait
  const int tid = threadIdx.x, l = tid & 63, j = l & 31, kh = l >> 5;
  const int gw = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (PTPB / 64) + (tid >> 6)));
  const int nwaves = gridDim.x * (PTPB / 64);
  // No MT19937 refill here: the episode's reset kernel (k_env_reset) regenerates every stale block
  // of each env's 4-block ring (env_dev.h, MT_BLOCKS), so each env starts the episode with three
  // fresh 624-word blocks in reserve beyond its active one — more than an episode draws (reset
  // 24-61 words, a step 0-18) — and RngT twists in-lane in the (correct, never observed) case
  // that an env exhausts the whole ring within one episode.
  // A per-step refill here cost the policy step up to 25 us in the draw-heavy early steps (every
  // stale env a 624-word twist serialised in its wave) and its first step ~100 us.
  stage_both<PTPB>(lds, Wc, Ww, tid);
  __syncthreads();
  const int R = c.N * c.nS * c.P;
  const int32_t *__restrict__ rows = B.rows;
  const int nc = __builtin_amdgcn_readfirstlane(rows[R]), nw = __builtin_amdgcn_readfirstlane(rows[R + 1]);
  // this launch's rows: all of both lists, or part `part`'s run of each (k_part_bounds)
  int c0 = 0, ncp = nc, w0 = nc, nwp = nw;
  if (nparts > 1) {
    const int wb = R + 2 + nparts + 1;
    c0 = __builtin_amdgcn_readfirstlane(rows[R + 2 + part]);
    ncp = __builtin_amdgcn_readfirstlane(rows[R + 3 + part]) - c0;
    const int w0r = __builtin_amdgcn_readfirstlane(rows[wb + part]);
    w0 = nc + w0r;
    nwp = __builtin_amdgcn_readfirstlane(rows[wb + part + 1]) - w0r;
  }
  const int tc = (ncp + 31) / 32, ntiles = tc + (nwp + 31) / 32;
  const ObsLayout L = obs_layout(c);
  // software pipeline over this wave's tiles: row indices two tiles ahead, the rows'
  // observation values one tile ahead, so the gathers overlap the MFMA work
  auto tile_row = [&](int tl, bool &ok) {
    const int hd = tl >= tc;
    const int a0 = hd ? w0 + 32 * (tl - tc) : c0 + 32 * tl, a1 = hd ? w0 + nwp : c0 + ncp;
    ok = tl < ntiles && a0 + j < a1;
    return ok ? rows[a0 + j] : 0;
  };
  auto raw_of = [&](int rr) {
    const int pp = rr % c.P, ii = (rr / c.P) % c.nS, ee = rr / (c.P * c.nS);
    return feat_raw(B.obs + (size_t)ee * L.obs_dim, L, ii, pp);
  };
  bool ok_cur, ok_nxt;
  int r_cur = tile_row(gw, ok_cur);
  int r_nxt = tile_row(gw + nwaves, ok_nxt);
  FeatRaw raw_cur = raw_of(r_cur);
  for (int tile = gw; tile < ntiles; tile += nwaves) {
    bool ok_2;
    const int r_2 = tile_row(tile + 2 * nwaves, ok_2);
    const FeatRaw raw_nxt = raw_of(r_nxt);
    const int head = tile >= tc;
    const float *Wl = lds + head * HEAD;
    const bool valid = ok_cur;
    const int r = r_cur;
    float f[NF_C + 1];
    const float ex = obs_car_ped_raw(raw_cur, f);
    f[NF_C] = 0.0f;
    r_cur = r_nxt;
    ok_cur = ok_nxt;
    r_nxt = r_2;
    ok_nxt = ok_2;
    raw_cur = raw_nxt;
    const int64_t fr = valid ? feat_row<V>(B, c.P, r) : -1;
    if (fr >= 0 && kh == 0) {
      float *fo = B.feat_c + fr * NF_C;
#pragma unroll
      for (int q = 0; q < NF_C; q++) fo[q] = f[q];
    }
    const float out = actor_tile(Wl, f, j, kh);
    if (valid && kh == 0 && !(L.scalable && ex == 0.0f)) {  // `if exist:` gate (:439)
      // ppo_heads.h finish_cont<LibmRollout>, restated (the mean is picked after the product: a call picks it before)
      const float t = mhppo_tanhf(out) * (head ? std_w : std_c);  // Model_PPO type 1 (:87-89)
      B.out_c[r] = t + (head ? mean_w : mean_c);
    }
  }
}

}  // namespace
