// mlp_gae.hip — GAE(lambda) targets over the rollout's time-major records (+ C-ABI):
//   k_gae_tm  the critics' forward and the backward lambda-return scan of every record in one
//             launch (mhppo_gae_tm; opt-in, Algo_PPO(gae_lambda=...)).
// A wave owns 32 consecutive records (the tile rows on the lanes, as in k_mlp_forward) and walks
// t = T-1 .. 0: step t's input tile is the contiguous run obs_tm[t][32 w .. 32 w + 31], forwarded
// through the record's critic on f32 MFMA in the rollout's arithmetic (mlp_infer_tile.h, so V is
// bit for bit mhppo_mlp_forward's), and the float64 recurrence of include/mhppo.h runs in the
// registers of the lower lane half.  Both critics' images stay in LDS; a critic none of the tile's
// used records belongs to is not forwarded (wave-wide ballot), a tile without a used record only
// writes its zeros.  Step t - 1's tile and reward are loaded while step t's MFMA chain runs (two
// input slots per wave).  A wave reads and writes only its own slots and its own records, in its
// own order: no block barrier after the images are staged, no atomics, nothing depends on the grid.
// A record's scan needs its own critic's values only, so while the tiles are too few to fill the
// SIMDs (small B: the launch lasts as long as one wave's serial t loop) a tile is served by two
// waves, one per critic, each scanning and writing the records of its critic (k_gae_tm `split`):
// the same operations per record, the same bits.
//
// Unused records (pos < 0) are still staged — their observation rows may hold anything, NaN
// included.  That cannot reach another record: the inputs are the MFMA's B operand, so output
// column j (tile row j) of every layer is a sum over products with input column j alone, and the
// permlane swap of the last layer exchanges the two halves of the SAME column.  An unused record's
// own V is discarded and its outputs are written as 0.
//
// k_gae_tm<true> (mhppo_gae_tm_len): record b has len_rec[b] steps (clamped to [0, T]).  That is a
// per-lane mask on `used` where the recurrence runs: at t >= len the record writes 0 and leaves
// A = nv = 0, so its scan starts from there at t = len - 1 (the early end is terminal).  The wave
// still walks all T steps; V_t is untouched.
//
// k_gae_tm<true, const float *> (mhppo_gae_tm_boot): the same with a bootstrap value per record, a
// truncated segment's V(s_L): nv = v_boot[b] immediately before step len - 1's delta, A = 0.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/mhppo.h"
#include "common.h"
#include "mlp_infer_terms.h"
#include "mlp_infer_tile.h"

using namespace mhppo;
using namespace mhppo::infer;

namespace {
// Launch shape, a function of B and of whether pos is given (never of the device or the data):
// four-wave blocks (two resident per CU by LDS: two waves per SIMD), one (tile, critic set) unit per
// wave, at most MAX_BLOCKS blocks walking the units grid-stride.  With pos (two critics), up to
// SPLIT_TILES tiles (half the 2048 wave slots) a tile is two units, one per critic; with pos == NULL
// there is one critic and nothing to split: a small B then has its tiles' serial loops as its only
// parallelism (256 tiles: 64 blocks).  (Smaller blocks for small B, to reach more CUs, were measured no faster: a wave has its
// SIMD to itself either way, and 64 threads stage the images more slowly.)
constexpr int GW = 4, MAX_BLOCKS = 512, SPLIT_TILES = MAX_BLOCKS * GW / 2;

// LDS ordering inside one wave (its own input slots): the DS queue is in order per wave, the
// fences keep the compiler from moving the accesses
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS: [critic0 image][critic1 image, if W1][2 GW input tiles]
// split (needs W1): unit u is tile u >> 1 with critic u & 1 alone; else unit u is tile u with both
// VB: nothing (mhppo_gae_tm / _len), or one const float * (v_boot: mhppo_gae_tm_boot).  A pack, so
// that without it the kernel is parameter for parameter the function it was before the bootstrap
// and compiles to the same instructions (profiles/bootstrap/kernel_diff.txt; called from a shared
// inlined body, k_gae_tm<false> and <true> came out with one v_add_f64's operands exchanged).
template <bool LEN, typename... VB>
__global__ void __launch_bounds__(64 * GW)
    k_gae_tm(const float *__restrict__ W0, const float *__restrict__ W1, int n_in, const float *__restrict__ obs_tm,
             const double *__restrict__ rew_tm, const int64_t *__restrict__ pos, const int8_t *__restrict__ bucket,
             int64_t B, int T, double gamma, double lambda, int split, float *__restrict__ ret_tm,
             float *__restrict__ value_tm, const int32_t *__restrict__ len_rec, VB... v_boot) {
  constexpr bool BOOT = sizeof...(VB) != 0;
  static_assert(!BOOT || LEN, "the bootstrap needs the lengths");
  extern __shared__ float lds[];
  const int tid = threadIdx.x, l = tid & 63, j = l & 31, kh = l >> 5, w = tid >> 6;
  const Img g = img_layout(n_in, 1);
  const int xt = xtile_floats(g);
  const float *L0 = lds, *L1 = lds + g.size;
  float *xa = lds + (W1 ? 2 : 1) * g.size + 2 * w * xt, *xb = xa + xt;
  stage_image<64 * GW>(lds, g, W0, n_in, 1, tid);
  if (W1) stage_image<64 * GW>(lds + g.size, g, W1, n_in, 1, tid);
  zero_x_pad(xa, g, n_in, l);
  zero_x_pad(xb, g, n_in, l);
  __syncthreads();  // the images; from here on the waves are independent
  const XStage xst = xstage_init(n_in, l);
  const int64_t ntiles = (B + 31) / 32, units = split ? 2 * ntiles : ntiles, stride = (int64_t)gridDim.x * GW,
                step = B * n_in;
  const double c = gamma * lambda;
  for (int64_t u = (int64_t)blockIdx.x * GW + w; u < units; u += stride) {
    const int64_t tile = split ? u >> 1 : u;
    const int only = split ? (int)(u & 1) : -1;  // the one critic this wave serves; -1: both
    const int64_t r0 = tile * 32, r = r0 + j;
    const int nr = B - r0 < 32 ? (int)(B - r0) : 32;
    bool used = j < nr, b1 = false;
    if (pos && used) {
      used = pos[r] >= 0;
      b1 = used && bucket[r] != 0;
    }
    // the wave's records: all of the tile, or those of its critic (unused ones go with critic 0);
    // mine: the lane that owns record r's scan and outputs
    int Lr = T;  // the record's steps
    if (LEN && j < nr) Lr = min(max(len_rec[r], 0), T);
    const bool own = only < 0 || (used ? (int)b1 == only : only == 0);
    const bool mine = kh == 0 && j < nr && own;
    const bool any0 = only != 1 && __builtin_amdgcn_ballot_w64(used && !b1) != 0,
               any1 = only != 0 && __builtin_amdgcn_ballot_w64(b1) != 0;
    if (!any0 && !any1) {
      if (mine)
        for (int t = 0; t < T; t++) {
          ret_tm[(int64_t)t * B + r] = 0.0f;
          if (value_tm) value_tm[(int64_t)t * B + r] = 0.0f;
        }
      continue;
    }
    float *xc = xa, *xn = xb;
    wave_sync();  // the previous tile's reads of xc
    stage_x(xc, g, xst, obs_tm + (int64_t)(T - 1) * step, r0, nr, n_in, l);
    double rw = mine && used ? rew_tm[(int64_t)(T - 1) * B + r] : 0.0;
    double vb = 0.0;  // BOOT: the value after the record's last step
    if constexpr (BOOT) {
      if (mine && used) vb = (double)(v_boot, ...)[r];
    }
    double A = 0.0, nv = 0.0;
#pragma unroll 1
    for (int t = T - 1; t >= 0; t--) {
      wave_sync();  // xc is staged
      // step t - 1's tile and reward, in flight behind this step's MFMA chain
      float pre[8];
      double rw_n = 0.0;
      const float *src = obs_tm + (int64_t)(t > 0 ? t - 1 : 0) * step + r0 * n_in;
      if (t > 0) {
        stage_x_issue(pre, src, nr, n_in, l);
        if (mine && used) rw_n = rew_tm[(int64_t)(t - 1) * B + r];
      }
      float vf = 0.0f;
      // one net at a time (k_ppo_diag: interleaved, both forwards' accumulators would be live at once)
      if (any0) {
        float z[1];
        tile_forward<1>(L0, g, xc, j, kh, z);
        if (!b1) vf = z[0];
        __builtin_amdgcn_sched_barrier(0);
      }
      if (any1) {
        float z[1];
        tile_forward<1>(L1, g, xc, j, kh, z);
        if (b1) vf = z[0];
        __builtin_amdgcn_sched_barrier(0);
      }
      if (t > 0) stage_x_land(xn, g, xst, pre, src, nr, n_in, l);
      if (mine) {
        float ret = 0.0f;
        if (used && (!LEN || t < Lr)) {
          const double v = (double)vf;
          if constexpr (BOOT) {
            if (t == Lr - 1) nv = vb;
          }
          const double d = (rw + gamma * nv) - v;
          A = d + c * A;
          ret = (float)(A + v);
          nv = v;
        } else {
          vf = 0.0f;
        }
        ret_tm[(int64_t)t * B + r] = ret;
        if (value_tm) value_tm[(int64_t)t * B + r] = vf;
      }
      rw = rw_n;
      float *x = xc;
      xc = xn;
      xn = x;
    }
  }
}

int check_critic(const mhppo_mlp *m, const char *what) {
  if (!m || !m->packed) return set_error(MHPPO_EINVAL, "mhppo_gae_tm: null pointer (%s)", what);
  if (m->kind != 0 || m->n_out != 1)
    return set_error(MHPPO_EINVAL, "mhppo_gae_tm: %s is kind %d with n_out %d, not a critic (kind 0, n_out 1)", what,
                     (int)m->kind, (int)m->n_out);
  if (m->n_in < 1 || m->n_in > N_IN_MAX)
    return set_error(MHPPO_EINVAL, "mhppo_gae_tm: %s n_in %d outside 1..%d", what, (int)m->n_in, N_IN_MAX);
  return MHPPO_OK;
}

LdsLimit g_lds_limit[3];  // the three instantiations' dynamic LDS above the default 64 KB (wide critics)

int launch(const float *W0, const float *W1, int n_in, const float *obs_tm, const double *rew_tm, const int64_t *pos,
           const int8_t *bucket, int64_t B, int T, double gamma, double lambda, float *ret_tm, float *value_tm,
           const int32_t *len_rec, const float *v_boot, hipStream_t s) {
  const Img g = img_layout(n_in, 1);
  const size_t shm = ((size_t)(W1 ? 2 : 1) * g.size + (size_t)2 * GW * xtile_floats(g)) * sizeof(float);
  const int split = W1 && n_tiles(B) <= SPLIT_TILES;
  const int64_t units = split ? 2 * n_tiles(B) : n_tiles(B);
  const int nb = (int)std::min<int64_t>((units + GW - 1) / GW, MAX_BLOCKS);
  if (v_boot) {
    const auto kern = k_gae_tm<true, const float *>;
    if (int rc = allow_dynamic_lds(reinterpret_cast<const void *>(kern), shm, g_lds_limit[2])) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(64 * GW), shm, s, W0, W1, n_in, obs_tm, rew_tm, pos,
                       bucket, B, T, gamma, lambda, split, ret_tm, value_tm, len_rec, v_boot);
    CHECK_HIP(hipGetLastError());
    return MHPPO_OK;
  }
  const auto kern = len_rec ? k_gae_tm<true> : k_gae_tm<false>;
  if (int rc = allow_dynamic_lds(reinterpret_cast<const void *>(kern), shm, g_lds_limit[len_rec ? 1 : 0])) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(64 * GW), shm, s, W0, W1, n_in, obs_tm, rew_tm, pos, bucket, B, T,
                     gamma, lambda, split, ret_tm, value_tm, len_rec);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

// the three entry points: len_rec == NULL is mhppo_gae_tm, v_boot == NULL mhppo_gae_tm_len
int gae_tm(const mhppo_mlp *critic0, const mhppo_mlp *critic1, const float *obs_tm, const double *rew_tm,
           const int64_t *pos, const int8_t *bucket, int64_t B, int32_t T, double gamma, double lambda, float *ret_tm,
           float *value_tm, const int32_t *len_rec, const float *v_boot, void *stream) {
  if (int rc = check_critic(critic0, "critic0")) return rc;
  if (pos || critic1) {
    if (int rc = check_critic(critic1, "critic1")) return rc;
    if (critic0->n_in != critic1->n_in)
      return set_error(MHPPO_EINVAL, "mhppo_gae_tm: critic0 n_in %d != critic1 n_in %d", (int)critic0->n_in,
                       (int)critic1->n_in);
  }
  if (pos && !bucket) return set_error(MHPPO_EINVAL, "mhppo_gae_tm: pos without bucket");
  if (T < 1) return set_error(MHPPO_EINVAL, "mhppo_gae_tm: T < 1");
  if (B < 0) return set_error(MHPPO_EINVAL, "mhppo_gae_tm: B < 0");
  if (v_boot && !len_rec) return set_error(MHPPO_EINVAL, "mhppo_gae_tm_boot: v_boot without len_rec");
  if (!(gamma >= 0.0 && gamma <= 1.0)) return set_error(MHPPO_EINVAL, "mhppo_gae_tm: gamma outside [0, 1]");
  if (!(lambda >= 0.0 && lambda <= 1.0)) return set_error(MHPPO_EINVAL, "mhppo_gae_tm: lambda outside [0, 1]");
  if (B == 0) return MHPPO_OK;
  if (!obs_tm || !rew_tm || !ret_tm) return set_error(MHPPO_EINVAL, "mhppo_gae_tm: null pointer");
  const float *W0 = critic0->packed, *W1 = pos ? critic1->packed : nullptr;  // pos == NULL: critic0 alone
  const int n_in = critic0->n_in;
  return launch(W0, W1, n_in, obs_tm, rew_tm, pos, bucket, B, T, gamma, lambda, ret_tm, value_tm, len_rec, v_boot,
                (hipStream_t)stream);
}
}  // namespace

extern "C" int mhppo_gae_tm(const mhppo_mlp *critic0, const mhppo_mlp *critic1, const float *obs_tm,
                            const double *rew_tm, const int64_t *pos, const int8_t *bucket, int64_t B, int32_t T,
                            double gamma, double lambda, float *ret_tm, float *value_tm, void *stream) {
  return gae_tm(critic0, critic1, obs_tm, rew_tm, pos, bucket, B, T, gamma, lambda, ret_tm, value_tm, nullptr, nullptr,
                stream);
}

extern "C" int mhppo_gae_tm_len(const mhppo_mlp *critic0, const mhppo_mlp *critic1, const float *obs_tm,
                                const double *rew_tm, const int64_t *pos, const int8_t *bucket, int64_t B, int32_t T,
                                double gamma, double lambda, float *ret_tm, float *value_tm, const int32_t *len_rec,
                                void *stream) {
  return gae_tm(critic0, critic1, obs_tm, rew_tm, pos, bucket, B, T, gamma, lambda, ret_tm, value_tm, len_rec, nullptr,
                stream);
}

extern "C" int mhppo_gae_tm_boot(const mhppo_mlp *critic0, const mhppo_mlp *critic1, const float *obs_tm,
                                 const double *rew_tm, const int64_t *pos, const int8_t *bucket, int64_t B, int32_t T,
                                 double gamma, double lambda, float *ret_tm, float *value_tm, const int32_t *len_rec,
                                 const float *v_boot, void *stream) {
  return gae_tm(critic0, critic1, obs_tm, rew_tm, pos, bucket, B, T, gamma, lambda, ret_tm, value_tm, len_rec, v_boot,
                stream);
}
