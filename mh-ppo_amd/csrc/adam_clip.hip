// adam_clip.hip — gradient-norm clipping and the Adam step of up to MHPPO_ADAM_MAX_NETS independent
// nets in one launch (+ C-ABI, mhppo_adam_clip; the arithmetic contract is include/mhppo.h's), and
// the same launch with a per-net gate decided on the device (mhppo_adam_clip_gated: the KL early stop).
// One block of 1024 threads per net: it folds the net's squared gradient in the fixed order of
// block_prims.h (k_fold<1024, 4> over the flat element index, across segment boundaries), forms
// the clip scale and steps the same net.  A net is 4 673 to 6 338 floats in the product: the launch
// is latency-bound, so a block keeps its loads four deep (the fold's four chains; four elements
// per thread and round in the step) and the whole segment table lives in the kernel arguments
// (scalar registers: finding an element's segment is a few compares, never a dependent load).
#include <hip/hip_runtime.h>

#include <math.h>

#include "../../include/mhppo.h"
#include "block_prims.h"
#include "common.h"

using namespace mhppo;

namespace {

constexpr int NT = 1024;
constexpr int CHAINS = 4;
constexpr int64_t N_TOTAL_MAX = (int64_t)1 << 30;  // the flat index and b + u NT stay in int

struct Seg {
  float *p;
  const float *g;
  float *m, *v, *step;
  int beg;  // the flat index of the segment's first element
};
struct Net {
  Seg seg[MHPPO_ADAM_MAX_SEGS];
  int n_seg, n;
  float stepf, a, q, c1, b2, c2, eps;
};
struct Args {
  Net net[MHPPO_ADAM_MAX_NETS];
};
// the gates of mhppo_adam_clip_gated, one per net (kl == nullptr: the net is not gated)
struct Gate {
  const double *kl;
  double limit;
  int *stop;
  int epoch;
};
struct Gates {
  Gate g[MHPPO_ADAM_MAX_NETS];
};
// the table, the gates, max_norm and norms all travel in the kernel arguments (include/mhppo.h)
static_assert(sizeof(Args) + sizeof(Gates) + sizeof(double) + sizeof(double *) <= 4096,
              "adam_clip: the kernel arguments outgrew the 4 KB of a launch");

struct Elem {
  float *p;
  const float *g;
  float *m, *v;
};

// The four addresses of flat element i (0 <= i < net.n): the last segment that begins at or before
// i (segments ascend; an empty one is passed over by its successor, which begins at the same index).
__device__ __forceinline__ Elem locate(const Net &net, int i) {
  Elem e = {net.seg[0].p, net.seg[0].g, net.seg[0].m, net.seg[0].v};
  int beg = 0;
#pragma unroll
  for (int s = 1; s < MHPPO_ADAM_MAX_SEGS; s++)
    if (s < net.n_seg && i >= net.seg[s].beg) {
      e = {net.seg[s].p, net.seg[s].g, net.seg[s].m, net.seg[s].v};
      beg = net.seg[s].beg;
    }
  const int o = i - beg;
  return {e.p + o, e.g + o, e.m + o, e.v + o};
}

// The block's work on its net: the fold, the norm, the clip scale, the step (both kernels below).
__device__ __forceinline__ void clip_and_step(const Net &net, double max_norm, double *norms) {
  const int n = net.n;
  double ss[1] = {strided_sum<NT, CHAINS>(
      [&](int i) {
        const double g = (double)*locate(net, i).g;
        return g * g;
      },
      n)};
  block_sum<NT>(ss);
  const double norm = sqrt(ss[0]);
  if (threadIdx.x == 0) {
    norms[blockIdx.x] = norm;
    for (int s = 0; s < net.n_seg; s++) *net.seg[s].step = net.stepf;
  }
  const double coef = max_norm / (norm + 1e-6);
  const float s = coef < 1.0 ? (float)coef : 1.0f;
  const float a = net.a, q = net.q, c1 = net.c1, b2 = net.b2, c2 = net.c2, eps = net.eps;
  for (int b = threadIdx.x; b < n; b += CHAINS * NT) {
    Elem e[CHAINS];
    float g[CHAINS], m[CHAINS], v[CHAINS], p[CHAINS];
#pragma unroll
    for (int u = 0; u < CHAINS; u++)
      if (b + u * NT < n) {
        e[u] = locate(net, b + u * NT);
        g[u] = *e[u].g, m[u] = *e[u].m, v[u] = *e[u].v, p[u] = *e[u].p;
      }
#pragma unroll
    for (int u = 0; u < CHAINS; u++)
      if (b + u * NT < n) {
        const float gs = g[u] * s;
        const float mn = m[u] + (gs - m[u]) * c1;
        const float vn = v[u] * b2 + (gs * gs) * c2;
        const float den = sqrtf(vn) / q + eps;  // correctly rounded (the Makefile pins the flag): compared bit for bit
        *e[u].m = mn;
        *e[u].v = vn;
        *e[u].p = p[u] - a * (mn / den);
      }
  }
}

__global__ void __launch_bounds__(NT) k_adam_clip(const Args args, double max_norm, double *norms) {
  clip_and_step(args.net[blockIdx.x], max_norm, norms);
}

// mhppo_adam_clip_gated.  A gated net's block first decides, alike in every thread, whether the net
// is open: *stop == 0 and kl[1] <= limit (a NaN fails the comparison).  Every thread reads *stop,
// then the barrier, then thread 0 alone may write it: no thread can read the word after the write.
// A closed net's block writes norms[k] = NaN, *stop = epoch if it was 0, and leaves: no gradient,
// parameter, moment or step of the net is read or written.
__global__ void __launch_bounds__(NT) k_adam_clip_gated(const Args args, double max_norm, double *norms,
                                                        const Gates gates) {
  const Gate &gt = gates.g[blockIdx.x];
  if (gt.kl) {
    const int stopped = *gt.stop;
    const bool open = stopped == 0 && gt.kl[1] <= gt.limit;
    __syncthreads();
    if (!open) {
      if (threadIdx.x == 0) {
        norms[blockIdx.x] = __builtin_nan("");
        if (stopped == 0) *gt.stop = gt.epoch;
      }
      return;
    }
  }
  clip_and_step(args.net[blockIdx.x], max_norm, norms);
}

}  // namespace

// The checks that both entry points share, and the launch table.
static int build_args(const mhppo_adam_net *nets, int32_t n_nets, double max_norm, const double *norms, Args &args) {
  if (!nets || !norms || n_nets < 0 || n_nets > MHPPO_ADAM_MAX_NETS)
    return set_error(MHPPO_EINVAL, "adam_clip: 0 .. %d nets, a table and norms", MHPPO_ADAM_MAX_NETS);
  if (!(max_norm > 0.0)) return set_error(MHPPO_EINVAL, "adam_clip: max_norm must be > 0 (inf allowed)");
  for (int k = 0; k < n_nets; k++) {
    const mhppo_adam_net &in = nets[k];
    Net &net = args.net[k];
    if (in.n_seg < 0 || in.n_seg > MHPPO_ADAM_MAX_SEGS)
      return set_error(MHPPO_EINVAL, "adam_clip: net %d has %d segments (0 .. %d)", k, in.n_seg, MHPPO_ADAM_MAX_SEGS);
    if (!(in.beta1 >= 0.0 && in.beta1 < 1.0 && in.beta2 >= 0.0 && in.beta2 < 1.0))
      return set_error(MHPPO_EINVAL, "adam_clip: net %d: betas must lie in [0, 1)", k);
    int64_t off = 0;
    for (int s = 0; s < in.n_seg; s++) {
      const mhppo_adam_seg &sg = in.seg[s];
      if (sg.n < 0 || !sg.step || (sg.n > 0 && (!sg.param || !sg.grad || !sg.exp_avg || !sg.exp_avg_sq)))
        return set_error(MHPPO_EINVAL, "adam_clip: net %d segment %d: n < 0 or a NULL pointer", k, s);
      if (sg.n > N_TOTAL_MAX - off) return set_error(MHPPO_EINVAL, "adam_clip: net %d holds more than 2^30 elements", k);
      net.seg[s] = {sg.param, sg.grad, sg.exp_avg, sg.exp_avg_sq, sg.step, (int)off};
      off += sg.n;
    }
    net.n_seg = in.n_seg;
    net.n = (int)off;
    net.stepf = (float)in.t;
    net.a = (float)in.alpha;
    net.q = (float)in.bias2;
    net.c1 = (float)(1.0 - in.beta1);
    net.b2 = (float)in.beta2;
    net.c2 = (float)(1.0 - in.beta2);
    net.eps = (float)in.eps;
  }
  return MHPPO_OK;
}

extern "C" int mhppo_adam_clip(const mhppo_adam_net *nets, int32_t n_nets, double max_norm, double *norms,
                               void *stream) {
  if (n_nets == 0) return MHPPO_OK;
  Args args = {};
  if (int rc = build_args(nets, n_nets, max_norm, norms, args)) return rc;
  hipLaunchKernelGGL(k_adam_clip, dim3(n_nets), dim3(NT), 0, (hipStream_t)stream, args, max_norm, norms);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}

extern "C" int mhppo_adam_clip_gated(const mhppo_adam_net *nets, int32_t n_nets, double max_norm, double *norms,
                                     const mhppo_adam_gate *gates, void *stream) {
  if (!gates) return mhppo_adam_clip(nets, n_nets, max_norm, norms, stream);
  if (n_nets == 0) return MHPPO_OK;
  Args args = {};
  if (int rc = build_args(nets, n_nets, max_norm, norms, args)) return rc;
  Gates gs = {};
  for (int k = 0; k < n_nets; k++) {
    const mhppo_adam_gate &in = gates[k];
    if (!in.kl) continue;
    if (!in.stop) return set_error(MHPPO_EINVAL, "adam_clip_gated: net %d is gated without a stop word", k);
    if (in.epoch < 1) return set_error(MHPPO_EINVAL, "adam_clip_gated: net %d: epoch %d < 1", k, (int)in.epoch);
    if (!(in.limit >= 0.0)) return set_error(MHPPO_EINVAL, "adam_clip_gated: net %d: limit must be >= 0 (inf allowed)", k);
    gs.g[k] = {in.kl, in.limit, in.stop, in.epoch};
  }
  hipLaunchKernelGGL(k_adam_clip_gated, dim3(n_nets), dim3(NT), 0, (hipStream_t)stream, args, max_norm, norms, gs);
  CHECK_HIP(hipGetLastError());
  return MHPPO_OK;
}
