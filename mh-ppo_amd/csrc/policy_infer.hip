// policy_infer.hip — the deterministic policy over observation rows, without an env (+ C-ABI):
//   k_policy_decide  the choice of every (row, slot, ped) triple: a_d and, optionally, the probabilities;
//   k_policy_act     the action vector of every row from its decisions: per slot the min over the
//                    pedestrians of the selected head's mean action (or the left-lane override),
//                    capped by (10 - V) / dt, and the lights.
// The rule is policy_rule.h's (what k_eval_step does before its env step).  Both kernels run 32-row
// tiles on f32 MFMA in the rollout's arithmetic (mlp_infer_tile.h), as k_mlp_forward / k_gae_tm do:
// four-wave blocks, the nets' permuted weight images staged once per block, a grid that is a
// function of M alone (at most MAX_BLOCKS blocks walking the tiles grid-stride), no atomics.  What
// is new is where a tile's input comes from: a wave stages the few observation rows its triples
// belong to (one contiguous run of `obs`, read 64 lanes wide) into LDS, and lane j < 32 builds
// triple j's feature row from that copy straight into row j of the wave's staged input tile (odd
// row stride: conflict-free stores).  Feature rows never touch HBM.  After the images are staged a
// wave touches only its own LDS slots and its own outputs: no block barrier, nothing depends on
// the grid.
//   k_policy_sample_decide / k_policy_sample_act  the training policy's stochastic rule
//                    (policy_sample_rule.h: what the collector draws) on the same structure, with
//                    the records the collector keeps: log-probabilities, feature rows, closest, exist.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/mhppo.h"
#include "common.h"
#include "mlp_infer_terms.h"
#include "mlp_infer_tile.h"
#include "policy_rule.h"
#include "policy_sample_rule.h"

using namespace mhppo;
using namespace mhppo::infer;
using namespace mhppo::policy;

namespace {
constexpr int PW = 4, MAX_BLOCKS = 512;
int n_blocks(int64_t tiles) { return (int)std::min<int64_t>((tiles + PW - 1) / PW, MAX_BLOCKS); }

struct NetArg {
  const float *W;
  float mean, std;
};

// LDS ordering inside one wave (its own slots): the DS queue is in order per wave, the fences keep
// the compiler from moving the accesses (k_gae_tm)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// observation rows [r_lo, r_lo + nrow) into the wave's staging: one contiguous run, 64 lanes wide
__device__ __forceinline__ void stage_obs(float *os, const float *__restrict__ obs, int64_t r_lo, int nrow, int od,
                                          int lane) {
  const float *src = obs + r_lo * od;
  const int n = nrow * od;
#pragma unroll 4
  for (int e = lane; e < n; e += 64) os[e] = src[e];
}

// obs_car_ped_d from the wave's observation staging straight into a row of its input tile.  The two
// LDS regions are disjoint, which the featurizer's plain pointers cannot say: without the restrict
// every feature's loads wait behind the previous feature's store, one LDS round trip per feature.
__device__ __forceinline__ void choice_features(const float *__restrict__ o, const ObsLayout &L, int i, int p,
                                                float *__restrict__ f) {
  obs_car_ped_d(o, L, i, p, f);
}

// a / b of a tile's first unit, in 32 bits when the launch's unit count allows (the 64-bit division is
// a long emulated sequence, paid per tile)
__device__ __forceinline__ int64_t tile_div(int64_t a, int b, bool small) {
  return small ? (int64_t)((uint32_t)a / (uint32_t)b) : a / b;
}

// The rows a tile's units [u0, u0 + n) (n <= 32 units, `per` units per observation row) can span
__host__ __device__ inline int span_rows(int n, int64_t per) { return (int)((n - 1) / per) + 2; }
// floats of one wave's observation staging, rounded to 16 bytes
__host__ __device__ inline int ostage_floats(int rows, int od) { return (rows * od + 3) / 4 * 4; }

// LDS: [image][PW input tiles][PW observation stagings]
// A tile is 32 consecutive triples q = (r S + i) P + p.
__global__ void __launch_bounds__(64 * PW)
    k_policy_decide(ObsLayout L, NetArg net, int dc, const float *__restrict__ obs, int64_t M,
                    int32_t *__restrict__ a_d, float *__restrict__ probs) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, l = tid & 63, j = l & 31, kh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the tile walk runs on the scalar unit
  const Img g = img_layout(dc, 2);
  const int xt = xtile_floats(g), SP = L.S * L.P, osz = ostage_floats(span_rows(32, SP), L.obs_dim);
  float *xs = lds + g.size + w * xt;
  float *os = lds + g.size + PW * xt + w * osz;
  stage_image<64 * PW>(lds, g, net.W, dc, 2, tid);
  zero_x_pad(xs, g, dc, l);
  __syncthreads();  // the image; from here on the waves are independent
  const int64_t Q = M * SP, ntiles = (Q + 31) / 32, stride = (int64_t)gridDim.x * PW;
  const bool small = Q <= INT32_MAX;
  // lane j's triple is the tile's first plus j = (ja SP + jb) triples, jb = ji P + jp: with the first
  // triple's (slot, ped) the lane's own follow by carries, no division per tile and lane
  const int ja = j / SP, jb = j - ja * SP, ji = jb / L.P, jp = jb - ji * L.P;
  for (int64_t tile = (int64_t)blockIdx.x * PW + w; tile < ntiles; tile += stride) {
    const int64_t q0 = tile * 32;
    const int nq = Q - q0 < 32 ? (int)(Q - q0) : 32;
    const int64_t r_lo = tile_div(q0, SP, small);
    const int off0 = (int)(q0 - r_lo * SP), oi = off0 / L.P, op = off0 - oi * L.P;
    wave_sync();  // the previous tile's reads of os and xs
    stage_obs(os, obs, r_lo, (off0 + nq - 1) / SP + 1, L.obs_dim, l);
    wave_sync();
    if (kh == 0) {
      float *xr = xs + j * g.S1;
      if (j < nq) {
        int p = jp + op, i = ji + oi, dr = ja;
        if (p >= L.P) p -= L.P, i++;
        if (i >= L.S) i -= L.S, dr++;
        choice_features(os + dr * L.obs_dim, L, i, p, xr);
      } else {
        for (int k = 0; k < dc; k++) xr[k] = 0.0f;
      }
    }
    wave_sync();  // the tile is staged
    float z[2];
    tile_forward<2>(lds, g, xs, j, kh, z);
    if (kh == 0 && j < nq) {
      const int64_t q = q0 + j;
      float p0, p1;
      a_d[q] = choice_of(z[0], z[1], p0, p1);
      if (probs) {
        probs[2 * q] = p0;
        probs[2 * q + 1] = p1;
      }
    }
  }
}

struct ActArgs {
  ObsLayout L;
  double dt, b00, b10;
};

// LDS: [cross image][wait image][PW input tiles][PW observation stagings][PW x 32 (cand, cap) doubles]
// A tile holds G = 32 / P whole (row, slot) groups u = r S + i of P triples each (lane j: group
// j / P, pedestrian j % P; the lanes past G P stage zeros), so a group's candidates meet in one wave.
__global__ void __launch_bounds__(64 * PW)
    k_policy_act(ActArgs A, NetArg cross, NetArg wait, const float *__restrict__ obs, const int32_t *__restrict__ a_d,
                 int64_t M, double *__restrict__ actions) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const ObsLayout &L = A.L;
  const int tid = threadIdx.x, l = tid & 63, j = l & 31, kh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave-uniform: the tile walk runs on the scalar unit
  const Img g = img_layout(NF_C, 1);
  const int xt = xtile_floats(g), S = L.S, P = L.P, G = 32 / P;
  const int osz = ostage_floats(span_rows(G, S), L.obs_dim);
  const float *Lc = lds, *Lw = lds + g.size;
  float *xs = lds + 2 * g.size + w * xt;
  float *os = lds + 2 * g.size + PW * xt + w * osz;
  double *cd = reinterpret_cast<double *>(lds + 2 * g.size + PW * xt + PW * osz) + w * 64;
  stage_image<64 * PW>(lds, g, cross.W, NF_C, 1, tid);
  stage_image<64 * PW>(lds + g.size, g, wait.W, NF_C, 1, tid);
  zero_x_pad(xs, g, NF_C, l);
  __syncthreads();  // the images; from here on the waves are independent
  const int gi = j / P, p = j - gi * P;  // the lane's group in the tile and its pedestrian
  const int ga = gi / S, gb = gi - ga * S;  // gi groups on = ga rows and gb slots on
  const int64_t U = M * S, ntiles = (U + G - 1) / G, stride = (int64_t)gridDim.x * PW;
  const bool small = U <= INT32_MAX;
  for (int64_t tile = (int64_t)blockIdx.x * PW + w; tile < ntiles; tile += stride) {
    const int64_t u0 = tile * G;
    const int nu = U - u0 < G ? (int)(U - u0) : G;
    const int64_t r_lo = tile_div(u0, S, small);
    const int off0 = (int)(u0 - r_lo * S);
    const bool live = kh == 0 && gi < nu;
    int i = gb + off0, dr = ga;  // the lane's slot and its row past r_lo, by carry
    if (i >= S) i -= S, dr++;
    const int64_t u = u0 + gi, r = r_lo + dr;
    // the triple's decision, issued ahead of the staging
    const int ad = live ? a_d[u * P + p] : 0;
    wave_sync();  // the previous tile's reads of os, xs and cd
    stage_obs(os, obs, r_lo, (off0 + nu - 1) / S + 1, L.obs_dim, l);
    wave_sync();
    float v = 0.0f;
    bool ovr = false;
    if (kh == 0) {
      float f[NF_C];
      if (live) {
        obs_car_ped(os + dr * L.obs_dim, L, i, p, f);
        v = f[0];
        ovr = f[7] != 0.0f;
      } else {
#pragma unroll
        for (int k = 0; k < NF_C; k++) f[k] = 0.0f;
      }
      float *xr = xs + j * g.S1;
#pragma unroll
      for (int k = 0; k < NF_C; k++) xr[k] = f[k];
    }
    const bool use_w = uses_wait(ad);
    // a head none of the tile's live, non-override triples uses is not forwarded
    const bool any_c = __builtin_amdgcn_ballot_w64(live && !ovr && !use_w) != 0,
               any_w = __builtin_amdgcn_ballot_w64(live && !ovr && use_w) != 0;
    wave_sync();  // the tile is staged
    float zf = 0.0f;
    // one net at a time (k_ppo_diag: interleaved, both forwards' accumulators would be live at once)
    if (any_c) {
      float z[1];
      tile_forward<1>(Lc, g, xs, j, kh, z);
      if (!use_w) zf = z[0];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (any_w) {
      float z[1];
      tile_forward<1>(Lw, g, xs, j, kh, z);
      if (use_w) zf = z[0];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (live) {
      const NetArg &m = use_w ? wait : cross;
      cd[2 * j] = ovr ? override_cand(v, A.dt, A.b00, A.b10) : head_cand(zf, m.mean, m.std);
      cd[2 * j + 1] = speed_cap(v, A.dt);
    }
    wave_sync();  // the group's candidates
    if (live && p == 0) {
      double a = A.b10;
      for (int k = 0; k < P; k++) fold_cand(a, cd[2 * (j + k)], cd[2 * (j + k) + 1]);
      double *row = actions + r * 2 * S;
      row[i] = a;
      row[S + i] = light_of(a_d + r * S * P, i);
    }
  }
}

// ---------------------------------------------------------------- the stochastic (training) policy
// policy_sample_rule.h's rule on the two kernels' structure: the same tiles, stagings and grid.  The
// only atomic is the status word's atomicOr (k_choice's), and it fires only on a NaN.
struct DecideOut {
  int32_t *a_d;
  float *logp_d, *probs, *feat_d;
  int32_t *closest;
  uint8_t *exist;
  uint32_t *status;
};

// LDS: [image][PW input tiles][PW observation stagings], as k_policy_decide.
// feat_d: a tile's nq feature rows are one contiguous run of nq dc floats, written from the LDS tile
// 64 lanes wide ((row, col) advanced per step as stage_x does: no division per element).
__global__ void __launch_bounds__(64 * PW)
    k_policy_sample_decide(ObsLayout L, NetArg net, int dc, const float *__restrict__ obs, int64_t M, SampleNoise nz,
                           DecideOut O) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, l = tid & 63, j = l & 31, kh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Img g = img_layout(dc, 2);
  const int xt = xtile_floats(g), SP = L.S * L.P, osz = ostage_floats(span_rows(32, SP), L.obs_dim);
  float *xs = lds + g.size + w * xt;
  float *os = lds + g.size + PW * xt + w * osz;
  stage_image<64 * PW>(lds, g, net.W, dc, 2, tid);
  zero_x_pad(xs, g, dc, l);
  __syncthreads();  // the image; from here on the waves are independent
  const int64_t Q = M * SP, ntiles = (Q + 31) / 32, stride = (int64_t)gridDim.x * PW;
  const bool small = Q <= INT32_MAX;
  const int ja = j / SP, jb = j - ja * SP, ji = jb / L.P, jp = jb - ji * L.P;
  const int fr0 = l / dc, fc0 = l - fr0 * dc, fsr = 64 / dc, fsc = 64 - fsr * dc;  // the feat_d run's walk
  for (int64_t tile = (int64_t)blockIdx.x * PW + w; tile < ntiles; tile += stride) {
    const int64_t q0 = tile * 32;
    const int nq = Q - q0 < 32 ? (int)(Q - q0) : 32;
    const int64_t r_lo = tile_div(q0, SP, small);
    const int off0 = (int)(q0 - r_lo * SP), oi = off0 / L.P, op = off0 - oi * L.P;
    const bool live = kh == 0 && j < nq;
    const int64_t q = q0 + j;
    // the triple's taped noise, issued ahead of the staging
    float u = 0.0f;
    int forced = 0;
    if (live && nz.forced) forced = nz.forced[q];
    else if (live && nz.tape) u = nz.tape[q];
    wave_sync();  // the previous tile's reads of os and xs
    stage_obs(os, obs, r_lo, (off0 + nq - 1) / SP + 1, L.obs_dim, l);
    wave_sync();
    int p = jp + op, i = ji + oi, dr = ja;
    if (p >= L.P) p -= L.P, i++;
    if (i >= L.S) i -= L.S, dr++;
    if (kh == 0) {
      float *xr = xs + j * g.S1;
      if (live) {
        choice_features(os + dr * L.obs_dim, L, i, p, xr);
      } else {
        for (int k = 0; k < dc; k++) xr[k] = 0.0f;
      }
    }
    wave_sync();  // the tile is staged
    if (O.feat_d) {
      float *dst = O.feat_d + q0 * dc;
      const int n = nq * dc;
      int row = fr0, col = fc0;
      for (int e = l; e < n; e += 64) {
        dst[e] = xs[row * g.S1 + col];
        row += fsr;
        col += fsc;
        if (col >= dc) col -= dc, row++;
      }
    }
    float z[2];
    tile_forward<2>(lds, g, xs, j, kh, z);
    if (live) {
      if (!nz.forced && !nz.tape) u = noise_uniform(nz, q, SP);
      float p0, p1, lp;
      O.a_d[q] = sample_choice(z[0], z[1], u, nz.forced != nullptr, forced, p0, p1, lp);
      O.logp_d[q] = lp;
      if (O.probs) {
        O.probs[2 * q] = p0;
        O.probs[2 * q + 1] = p1;
      }
      if (probs_nan(p0, p1) && O.status) atomicOr(O.status, 1u);
      if (p == 0) {
        const float *o = os + dr * L.obs_dim;
        const int64_t s = (r_lo + dr) * L.S + i;
        O.closest[s] = closest_ped_d(o, L, i);
        O.exist[s] = slot_exist(o, L, i);
      }
    }
  }
}

struct SampleActOut {
  double *actions;
  float *act, *logp, *feat_c;
  uint32_t *status;
};

// LDS: [cross image][wait image][PW input tiles][PW observation stagings][PW x (32 candidates, 32 sel,
// 64 normals)]
// Tiles of G = 32 / P whole (row, slot) groups, as k_policy_act.  The group's first lane folds its P
// candidates (a ballot carries which take part), samples, and stores the group's records; feat_c: the
// tile's nu selected feature rows are one contiguous run of nu x 13 floats, written from the LDS tile.
// The Philox normals are drawn 64 at a time, one per lane, for the wave's next 64 / G tiles (a tile
// needs only G of them: drawn per tile, the Box-Muller would run with G of 64 lanes busy).
__global__ void __launch_bounds__(64 * PW)
    k_policy_sample_act(ObsLayout L, NetArg cross, NetArg wait, const float *__restrict__ obs,
                        const int32_t *__restrict__ a_d, const int32_t *__restrict__ closest, int64_t M, SampleNoise nz,
                        SampleActOut O) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, l = tid & 63, j = l & 31, kh = l >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Img g = img_layout(NF_C, 1);
  const int xt = xtile_floats(g), S = L.S, P = L.P, G = 32 / P;
  const int osz = ostage_floats(span_rows(G, S), L.obs_dim);
  const float *Lc = lds, *Lw = lds + g.size;
  float *xs = lds + 2 * g.size + w * xt;
  float *os = lds + 2 * g.size + PW * xt + w * osz;
  float *cd = lds + 2 * g.size + PW * xt + PW * osz + w * 128;
  int *sl = reinterpret_cast<int *>(cd + 32);
  float *nl = cd + 64;
  stage_image<64 * PW>(lds, g, cross.W, NF_C, 1, tid);
  stage_image<64 * PW>(lds + g.size, g, wait.W, NF_C, 1, tid);
  zero_x_pad(xs, g, NF_C, l);
  __syncthreads();  // the images; from here on the waves are independent
  const int gi = j / P, p = j - gi * P;
  const int ga = gi / S, gb = gi - ga * S;
  const int64_t U = M * S, ntiles = (U + G - 1) / G, stride = (int64_t)gridDim.x * PW;
  const bool small = U <= INT32_MAX;
  const int B = 64 / G, tb = l / G, tg = l - tb * G;  // lane l draws for group tg of the wave's tb-th tile on
  int nb = 0;                                         // the wave's tiles since the last draw, < B
  for (int64_t tile = (int64_t)blockIdx.x * PW + w; tile < ntiles; tile += stride) {
    const int64_t u0 = tile * G;
    const int nu = U - u0 < G ? (int)(U - u0) : G;
    const int64_t r_lo = tile_div(u0, S, small);
    const int off0 = (int)(u0 - r_lo * S);
    const bool live = kh == 0 && gi < nu, head = live && p == 0;
    int i = gb + off0, dr = ga;
    if (i >= S) i -= S, dr++;
    const int64_t u = u0 + gi, r = r_lo + dr;
    // the triple's decision and the group's taped noise and light, issued ahead of the staging
    const int ad = live ? a_d[u * P + p] : 0;
    float eps = 0.0f;
    double light = 0.0;
    if (head) {
      if (nz.tape) eps = nz.tape[u];
      light = sample_light(a_d + r * S * P, P, i, closest[u]);
    }
    wave_sync();  // the previous tile's reads of os, xs, cd, sl and nl
    if (!nz.tape && nb == 0) {
      const int64_t tu = (tile + tb * stride) * G + tg;
      if (tb < B && tu < U) nl[l] = noise_normal(nz, tu, S);
    }
    stage_obs(os, obs, r_lo, (off0 + nu - 1) / S + 1, L.obs_dim, l);
    wave_sync();
    bool gate = false;
    if (kh == 0) {
      float f[NF_C];
      if (live) {
        const float *o = os + dr * L.obs_dim;
        obs_car_ped(o, L, i, p, f);
        gate = ped_gate(o, L, p);
      } else {
#pragma unroll
        for (int k = 0; k < NF_C; k++) f[k] = 0.0f;
      }
      float *xr = xs + j * g.S1;
#pragma unroll
      for (int k = 0; k < NF_C; k++) xr[k] = f[k];
    }
    const bool use_w = uses_wait(ad);
    // a head none of the tile's live triples uses is not forwarded (a gated-out triple only loses its
    // place in the fold)
    const bool any_c = __builtin_amdgcn_ballot_w64(live && !use_w) != 0,
               any_w = __builtin_amdgcn_ballot_w64(live && use_w) != 0;
    const uint32_t gmask = (uint32_t)__builtin_amdgcn_ballot_w64(gate);  // lanes 0 .. 31: kh == 0
    wave_sync();  // the tile is staged
    float zf = 0.0f;
    if (any_c) {
      float z[1];
      tile_forward<1>(Lc, g, xs, j, kh, z);
      if (!use_w) zf = z[0];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (any_w) {
      float z[1];
      tile_forward<1>(Lw, g, xs, j, kh, z);
      if (use_w) zf = z[0];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (live) {
      const NetArg &m = use_w ? wait : cross;
      cd[j] = finish_cont<LibmRollout>(zf, m.mean, m.std);
    }
    wave_sync();  // the group's candidates
    if (head) {
      float loc = 2.0f;  // torch.tensor(car_b[1, 0])
      int sel = 0;
      for (int k = 0; k < P; k++)
        if ((gmask >> (j + k)) & 1u) fold_sample(loc, sel, cd[j + k], k);
      if (loc != loc && O.status) atomicOr(O.status, 2u);
      if (!nz.tape) eps = nl[nb * G + gi];
      const float a = mvn_sample(loc, eps);
      O.act[u] = a;
      O.logp[u] = mvn_logp(a, loc);
      double *row = O.actions + r * 2 * S;
      row[i] = (double)a;
      row[S + i] = light;
      sl[gi] = j + sel;  // the tile row of the selected pedestrian's features
    }
    if (O.feat_c) {
      wave_sync();  // sl
      float *dst = O.feat_c + u0 * NF_C;
      for (int e = l; e < nu * NF_C; e += 64) {
        const int gq = e / NF_C, k = e - gq * NF_C;
        dst[e] = xs[sl[gq] * g.S1 + k];
      }
    }
    nb = nb + 1 == B ? 0 : nb + 1;
  }
}

int check_policy_net(const mhppo_mlp *m, int kind, int n_in, int n_out, const char *what) {
  if (!m || !m->packed) return set_error(MHPPO_EINVAL, "%s: null pointer", what);
  if (m->kind != kind) return set_error(MHPPO_EINVAL, "%s: kind %d, not %d", what, (int)m->kind, kind);
  if (m->n_in != n_in) return set_error(MHPPO_EINVAL, "%s: n_in %d, this config needs %d", what, (int)m->n_in, n_in);
  if (m->n_out != n_out) return set_error(MHPPO_EINVAL, "%s: n_out %d, not %d", what, (int)m->n_out, n_out);
  if (n_in < 1 || n_in > N_IN_MAX)
    return set_error(MHPPO_EINVAL, "%s: n_in %d outside 1..%d", what, n_in, N_IN_MAX);
  return MHPPO_OK;
}

int check_cfg(const mhppo_env_cfg *cfg, Cfg &c, const char *what) {
  if (const char *why = cfg_from(cfg, c)) return set_error(MHPPO_EINVAL, "%s: %s", what, why);
  return MHPPO_OK;
}

LdsLimit g_decide_lds, g_act_lds, g_sdecide_lds, g_sact_lds;

// a launch's noise from the C-ABI struct (NULL: refused by the callers)
SampleNoise noise_of(const mhppo_policy_noise *n) {
  return SampleNoise{n->tape, n->forced, n->key, n->first_env, n->t};
}
}  // namespace

extern "C" {

int mhppo_policy_dims(const mhppo_env_cfg *cfg, int32_t out[4]) {
  Cfg c;
  if (int rc = check_cfg(cfg, c, "mhppo_policy_dims")) return rc;
  if (!out) return set_error(MHPPO_EINVAL, "mhppo_policy_dims: null pointer");
  dims_of(c, out);
  return MHPPO_OK;
}

int mhppo_policy_decide(const mhppo_env_cfg *cfg, const mhppo_mlp *actor_choice, const float *obs, int64_t M,
                        int32_t *a_d, float *probs, void *stream) {
  Cfg c;
  if (int rc = check_cfg(cfg, c, "mhppo_policy_decide")) return rc;
  const int dc = choice_dim(c);
  if (int rc = check_policy_net(actor_choice, 2, dc, 2, "mhppo_policy_decide actor_choice")) return rc;
  if (M < 0) return set_error(MHPPO_EINVAL, "mhppo_policy_decide: M < 0");
  if (M == 0) return MHPPO_OK;
  if (!obs || !a_d) return set_error(MHPPO_EINVAL, "mhppo_policy_decide: null pointer");
  if ((uintptr_t)obs % 4) return set_error(MHPPO_EINVAL, "mhppo_policy_decide: obs is not 4-byte aligned");
  const ObsLayout L = obs_layout(c);
  const int64_t SP = (int64_t)c.nS * c.P;
  if (M > INT64_MAX / 64 / SP) return set_error(MHPPO_EINVAL, "mhppo_policy_decide: M too large");
  const Img g = img_layout(dc, 2);
  const size_t shm =
      ((size_t)g.size + (size_t)PW * xtile_floats(g) + (size_t)PW * ostage_floats(span_rows(32, SP), c.obs_dim)) *
      sizeof(float);
  if (int rc = allow_dynamic_lds(reinterpret_cast<const void *>(k_policy_decide), shm, g_decide_lds)) return rc;
  const NetArg net{actor_choice->packed, 0.0f, 1.0f};
  const int nb = n_blocks((M * SP + 31) / 32);
  hipLaunchKernelGGL(k_policy_decide, dim3((unsigned)nb), dim3(64 * PW), shm, (hipStream_t)stream, L, net, dc, obs, M,
                     a_d, probs);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_policy_act(const mhppo_env_cfg *cfg, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                     const float *obs, const int32_t *a_d, int64_t M, double *actions, void *stream) {
  Cfg c;
  if (int rc = check_cfg(cfg, c, "mhppo_policy_act")) return rc;
  if (c.P > MAX_P) return set_error(MHPPO_EINVAL, "mhppo_policy_act: nb_ped %d > %d", c.P, MAX_P);
  if (int rc = check_policy_net(actor_cross, 1, NF_C, 1, "mhppo_policy_act actor_cross")) return rc;
  if (int rc = check_policy_net(actor_wait, 1, NF_C, 1, "mhppo_policy_act actor_wait")) return rc;
  if (M < 0) return set_error(MHPPO_EINVAL, "mhppo_policy_act: M < 0");
  if (M == 0) return MHPPO_OK;
  if (!obs || !a_d || !actions) return set_error(MHPPO_EINVAL, "mhppo_policy_act: null pointer");
  if ((uintptr_t)obs % 4) return set_error(MHPPO_EINVAL, "mhppo_policy_act: obs is not 4-byte aligned");
  if (M > INT64_MAX / 64 / ((int64_t)c.nS * c.P)) return set_error(MHPPO_EINVAL, "mhppo_policy_act: M too large");
  ActArgs A{obs_layout(c), c.dt, c.b00, c.b10};
  const int G = 32 / c.P;
  const Img g = img_layout(NF_C, 1);
  const size_t shm =
      ((size_t)2 * g.size + (size_t)PW * xtile_floats(g) + (size_t)PW * ostage_floats(span_rows(G, c.nS), c.obs_dim)) *
          sizeof(float) +
      (size_t)PW * 64 * sizeof(double);
  if (int rc = allow_dynamic_lds(reinterpret_cast<const void *>(k_policy_act), shm, g_act_lds)) return rc;
  const NetArg nc{actor_cross->packed, actor_cross->mean, actor_cross->std},
      nw{actor_wait->packed, actor_wait->mean, actor_wait->std};
  const int nb = n_blocks((M * c.nS + G - 1) / G);
  hipLaunchKernelGGL(k_policy_act, dim3((unsigned)nb), dim3(64 * PW), shm, (hipStream_t)stream, A, nc, nw, obs, a_d, M,
                     actions);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_policy_sample_decide(const mhppo_env_cfg *cfg, const mhppo_mlp *actor_choice, const float *obs, int64_t M,
                               const mhppo_policy_noise *noise, int32_t *a_d, float *logp_d, float *probs,
                               float *feat_d, int32_t *closest, uint8_t *exist, uint32_t *status, void *stream) {
  Cfg c;
  if (int rc = check_cfg(cfg, c, "mhppo_policy_sample_decide")) return rc;
  const int dc = choice_dim(c);
  if (int rc = check_policy_net(actor_choice, 2, dc, 2, "mhppo_policy_sample_decide actor_choice")) return rc;
  if (M < 0) return set_error(MHPPO_EINVAL, "mhppo_policy_sample_decide: M < 0");
  if (!noise) return set_error(MHPPO_EINVAL, "mhppo_policy_sample_decide: null pointer");
  if (noise->tape && noise->forced)
    return set_error(MHPPO_EINVAL, "mhppo_policy_sample_decide: noise: a tape and forced decisions, one at most");
  if (M == 0) return MHPPO_OK;
  if (!obs || !a_d || !logp_d || !closest || !exist)
    return set_error(MHPPO_EINVAL, "mhppo_policy_sample_decide: null pointer");
  if ((uintptr_t)obs % 4) return set_error(MHPPO_EINVAL, "mhppo_policy_sample_decide: obs is not 4-byte aligned");
  const ObsLayout L = obs_layout(c);
  const int64_t SP = (int64_t)c.nS * c.P;
  if (M > INT64_MAX / 64 / SP / dc) return set_error(MHPPO_EINVAL, "mhppo_policy_sample_decide: M too large");
  const Img g = img_layout(dc, 2);
  const size_t shm =
      ((size_t)g.size + (size_t)PW * xtile_floats(g) + (size_t)PW * ostage_floats(span_rows(32, SP), c.obs_dim)) *
      sizeof(float);
  if (int rc = allow_dynamic_lds(reinterpret_cast<const void *>(k_policy_sample_decide), shm, g_sdecide_lds)) return rc;
  const NetArg net{actor_choice->packed, 0.0f, 1.0f};
  const DecideOut O{a_d, logp_d, probs, feat_d, closest, exist, status};
  const int nb = n_blocks((M * SP + 31) / 32);
  hipLaunchKernelGGL(k_policy_sample_decide, dim3((unsigned)nb), dim3(64 * PW), shm, (hipStream_t)stream, L, net, dc,
                     obs, M, noise_of(noise), O);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

int mhppo_policy_sample_act(const mhppo_env_cfg *cfg, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                            const float *obs, const int32_t *a_d, const int32_t *closest, int64_t M,
                            const mhppo_policy_noise *noise, double *actions, float *act, float *logp, float *feat_c,
                            uint32_t *status, void *stream) {
  Cfg c;
  if (int rc = check_cfg(cfg, c, "mhppo_policy_sample_act")) return rc;
  if (c.P > MAX_P) return set_error(MHPPO_EINVAL, "mhppo_policy_sample_act: nb_ped %d > %d", c.P, MAX_P);
  if (int rc = check_policy_net(actor_cross, 1, NF_C, 1, "mhppo_policy_sample_act actor_cross")) return rc;
  if (int rc = check_policy_net(actor_wait, 1, NF_C, 1, "mhppo_policy_sample_act actor_wait")) return rc;
  if (M < 0) return set_error(MHPPO_EINVAL, "mhppo_policy_sample_act: M < 0");
  if (!noise) return set_error(MHPPO_EINVAL, "mhppo_policy_sample_act: null pointer");
  if (noise->forced) return set_error(MHPPO_EINVAL, "mhppo_policy_sample_act: noise: forced decisions belong to decide");
  if (!noise->tape && noise->t < 0) return set_error(MHPPO_EINVAL, "mhppo_policy_sample_act: noise: t < 0");
  if (M == 0) return MHPPO_OK;
  if (!obs || !a_d || !closest || !actions || !act || !logp)
    return set_error(MHPPO_EINVAL, "mhppo_policy_sample_act: null pointer");
  if ((uintptr_t)obs % 4) return set_error(MHPPO_EINVAL, "mhppo_policy_sample_act: obs is not 4-byte aligned");
  if (M > INT64_MAX / 64 / ((int64_t)c.nS * c.P) / NF_C)
    return set_error(MHPPO_EINVAL, "mhppo_policy_sample_act: M too large");
  const ObsLayout L = obs_layout(c);
  const int G = 32 / c.P;
  const Img g = img_layout(NF_C, 1);
  const size_t shm =
      ((size_t)2 * g.size + (size_t)PW * xtile_floats(g) + (size_t)PW * ostage_floats(span_rows(G, c.nS), c.obs_dim) +
       (size_t)PW * 128) *
      sizeof(float);
  if (int rc = allow_dynamic_lds(reinterpret_cast<const void *>(k_policy_sample_act), shm, g_sact_lds)) return rc;
  const NetArg nc{actor_cross->packed, actor_cross->mean, actor_cross->std},
      nw{actor_wait->packed, actor_wait->mean, actor_wait->std};
  const SampleActOut O{actions, act, logp, feat_c, status};
  const int nb = n_blocks((M * c.nS + G - 1) / G);
  hipLaunchKernelGGL(k_policy_sample_act, dim3((unsigned)nb), dim3(64 * PW), shm, (hipStream_t)stream, L, nc, nw, obs,
                     a_d, closest, M, noise_of(noise), O);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

}  // extern "C"
