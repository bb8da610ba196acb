// boot_values.hip — the bootstrap values of truncated segments of an external rollout (+ C-ABI):
//   k_boot_values  V(s_L) of every segment whose episode was cut, not ended (mhppo_boot_values;
//                  opt-in, ExternalRollout(bootstrap=True)).
// The rule is per segment s = r S + i (include/mhppo.h): its stream r gives the effective length L
// and whether the end was a truncation, its record column col = rec_of[s] the critic (bucket[col])
// and the successor row -- record L of that column for L < k, the segment's row of feat_tail for
// L == k.  A wave owns 32 consecutive segments (the tile rows on the lanes, as in k_mlp_forward):
// lane j < 32 fetches its own segment's row into the wave's staged input tile -- a gather: the
// columns of consecutive present segments are adjacent, but L differs per stream -- and the tile
// goes through the critic on f32 MFMA in the rollout's arithmetic (mlp_infer_tile.h), so the
// value is bit for bit mhppo_mlp_forward's.  Both critics' images stay in LDS; a critic no selected
// segment of the tile belongs to is not forwarded (wave-wide ballot), a tile without a selected
// segment only writes its zeros.  A wave reads and writes only its own input tile and its own
// columns: no block barrier after the images are staged, no atomics, and the grid is a function of
// M S alone.
//
// A row that the rule does not select is never read: its tile row is staged as zeros, and even a
// staged NaN could not reach another segment -- the inputs are the MFMA's B operand, so output
// column j of every layer is a sum over products with input column j alone (mlp_gae.hip).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/mhppo.h"
#include "common.h"
#include "mlp_infer_terms.h"
#include "mlp_infer_tile.h"

using namespace mhppo;
using namespace mhppo::infer;

namespace {
// Four-wave blocks, one tile per wave and step, at most MAX_BLOCKS blocks walking the tiles
// grid-stride (two blocks per CU on 256 CUs; config 3's 8192 tiles are four per wave)
constexpr int GW = 4, MAX_BLOCKS = 512;

// LDS ordering inside one wave (its own input tile): the DS queue is in order per wave, the fences
// keep the compiler from moving the accesses
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS: [critic0 image][critic1 image][GW input tiles]
__global__ void __launch_bounds__(64 * GW)
    k_boot_values(const float *__restrict__ W0, const float *__restrict__ W1, int n_in,
                  const int64_t *__restrict__ pos, const int8_t *__restrict__ bucket,
                  const int32_t *__restrict__ rec_of, const int32_t *__restrict__ len,
                  const uint8_t *__restrict__ trunc, int64_t NS, int S, int k, int cut_truncates,
                  const float *__restrict__ obs_tm, const float *__restrict__ feat_tail, float *__restrict__ v_boot) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, l = tid & 63, j = l & 31, kh = l >> 5, w = tid >> 6;
  const Img g = img_layout(n_in, 1);
  const float *L0 = lds, *L1 = lds + g.size;
  float *xs = lds + 2 * g.size + w * xtile_floats(g);
  stage_image<64 * GW>(lds, g, W0, n_in, 1, tid);
  stage_image<64 * GW>(lds + g.size, g, W1, n_in, 1, tid);
  zero_x_pad(xs, g, n_in, l);
  __syncthreads();  // the images; from here on the waves are independent
  const int64_t ntiles = (NS + 31) / 32, stride = (int64_t)gridDim.x * GW, step = NS * n_in;
  for (int64_t tile = (int64_t)blockIdx.x * GW + w; tile < ntiles; tile += stride) {
    // both lane halves evaluate the rule of segment s (the ballots and the forward are wave-wide);
    // the lower half fetches the row and writes the value
    const int64_t s = tile * 32 + j;
    int64_t col = -1;
    if (s < NS) col = rec_of ? (int64_t)rec_of[s] : s;
    bool sel = false, b1 = false;
    const float *row = nullptr;
    if (col >= 0) {
      const int64_t r = s / S;
      const int ln = len[r];
      const bool ended = ln >= 1 && ln <= k;
      const int L = ended ? ln : k;
      const bool tr = ended ? trunc[r] != 0 : cut_truncates != 0;
      sel = pos[col] >= 0 && tr && (L < k || feat_tail);
      if (sel) {
        b1 = bucket[col] != 0;
        row = L < k ? obs_tm + (int64_t)L * step + col * n_in : feat_tail + s * n_in;
      }
    }
    const bool any0 = __builtin_amdgcn_ballot_w64(sel && !b1) != 0, any1 = __builtin_amdgcn_ballot_w64(b1) != 0;
    const bool mine = kh == 0 && col >= 0;
    if (!any0 && !any1) {
      if (mine) v_boot[col] = 0.0f;
      continue;
    }
    wave_sync();  // the previous tile's reads of xs
    if (kh == 0) {
      float *xr = xs + j * g.S1;
      // eight loads in flight per lane, then their stores (13 inputs: two batches)
#pragma unroll 1
      for (int c0 = 0; c0 < n_in; c0 += 8) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; q++) v[q] = sel && c0 + q < n_in ? row[c0 + q] : 0.0f;
#pragma unroll
        for (int q = 0; q < 8; q++)
          if (c0 + q < n_in) xr[c0 + q] = v[q];
      }
    }
    wave_sync();  // xs is staged
    float vf = 0.0f;
    // one net at a time (k_gae_tm: interleaved, both forwards' accumulators would be live at once)
    if (any0) {
      float z[1];
      tile_forward<1>(L0, g, xs, j, kh, z);
      if (sel && !b1) vf = z[0];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (any1) {
      float z[1];
      tile_forward<1>(L1, g, xs, j, kh, z);
      if (b1) vf = z[0];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (mine) v_boot[col] = vf;
  }
}

int check_critic(const mhppo_mlp *m, const char *what) {
  if (!m || !m->packed) return set_error(MHPPO_EINVAL, "mhppo_boot_values: null pointer (%s)", what);
  if (m->kind != 0 || m->n_out != 1)
    return set_error(MHPPO_EINVAL, "mhppo_boot_values: %s is kind %d with n_out %d, not a critic (kind 0, n_out 1)",
                     what, (int)m->kind, (int)m->n_out);
  if (m->n_in < 1 || m->n_in > N_IN_MAX)
    return set_error(MHPPO_EINVAL, "mhppo_boot_values: %s n_in %d outside 1..%d", what, (int)m->n_in, N_IN_MAX);
  return MHPPO_OK;
}

LdsLimit g_lds_limit;  // k_boot_values' dynamic LDS above the default 64 KB (wide critics)
}  // namespace

extern "C" int mhppo_boot_values(const mhppo_mlp *critic0, const mhppo_mlp *critic1, const int64_t *pos,
                                 const int8_t *bucket, const int32_t *rec_of, const int32_t *len,
                                 const uint8_t *trunc, int64_t M, int32_t S, int32_t k, int32_t cut_truncates,
                                 const float *obs_tm, const float *feat_tail, float *v_boot, void *stream) {
  if (int rc = check_critic(critic0, "critic0")) return rc;
  if (int rc = check_critic(critic1, "critic1")) return rc;
  if (critic0->n_in != critic1->n_in)
    return set_error(MHPPO_EINVAL, "mhppo_boot_values: critic0 n_in %d != critic1 n_in %d", (int)critic0->n_in,
                     (int)critic1->n_in);
  if (M < 0 || S < 1 || M > INT32_MAX / (int64_t)S)
    return set_error(MHPPO_EINVAL, "mhppo_boot_values: M < 0, S < 1 or M S > 2^31 - 1");
  if (k < 1) return set_error(MHPPO_EINVAL, "mhppo_boot_values: k < 1");
  if (M == 0) return MHPPO_OK;
  if (!pos || !bucket || !len || !trunc || !obs_tm || !v_boot)
    return set_error(MHPPO_EINVAL, "mhppo_boot_values: a NULL pointer other than rec_of and feat_tail");
  const int n_in = critic0->n_in;
  const int64_t NS = M * S;
  const Img g = img_layout(n_in, 1);
  const size_t shm = ((size_t)2 * g.size + (size_t)GW * xtile_floats(g)) * sizeof(float);
  if (int rc = allow_dynamic_lds(reinterpret_cast<const void *>(k_boot_values), shm, g_lds_limit)) return rc;
  const int nb = (int)std::min<int64_t>((n_tiles(NS) + GW - 1) / GW, MAX_BLOCKS);
  hipLaunchKernelGGL(k_boot_values, dim3((unsigned)nb), dim3(64 * GW), shm, (hipStream_t)stream, critic0->packed,
                     critic1->packed, n_in, pos, bucket, rec_of, len, trunc, NS, (int)S, (int)k, (int)cut_truncates,
                     obs_tm, feat_tail, v_boot);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}
