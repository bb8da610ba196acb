// rollout_step.h — the per-step env kernels of the collector, one lane per env:
//   RecStage          a wave's LDS run for the compact layout's step records
//   sample_env_body   min over pedestrians, MVN draw, log-prob, rollout-buffer writes, then the env
//                     step itself (env_body.h) and the episodic min
//   k_sample_env      that body on the generic env view, k_sample_env_r on the register view
//   k_eval_step       the deterministic evaluation step (Env_rollout.iterations)
//   k_fill_f64        the episodic minima's reset
// (rec_map, the record index of a segment, is rollout_policy.h's.)
// Part of the rollout.hip translation unit (one anonymous namespace); not for inclusion elsewhere.
#pragma once
#include "env_body.h"
#include "launch1d.h"
#include "ppo_heads.h"
#include "rollout_dev.h"
#include "rollout_policy.h"

namespace {
using namespace mhppo;

// The compact layout's step records of one full wave (the scalable env): its 64 envs' present
// segments are the records [R0, R0 + K) (R0 = the existing segments before its first env,
// mhppo_rollout_bufs.rec_of[N S + e]); each lane puts its slots' act / logp / rew at (record - R0)
// in the wave's LDS run, and the wave writes the run as lane-contiguous stores.  (Stored per lane,
// the records' 4- and 8-byte values land scattered over the run and leave as partial lines:
// +2 % HBM bytes and +4 % time for the step kernel at config 4.)
template <int CNS>
struct RecStage {
  float act[64 * CNS], logp[64 * CNS];
  double rew[64 * CNS];
};
template <int CNS>
__device__ __forceinline__ RecStage<CNS> *rec_stage_wave() {
  __shared__ RecStage<CNS> st[TPB / 64];
  return &st[(threadIdx.x >> 6) & (TPB / 64 - 1)];
}

// one lane per env: select/min over peds, MVN sample, buffers, env step, episodic min.
// All of this lane's rollout inputs are read before any buffer write so the loads
// issue as one batch; EV is the generic or the register env view.
template <class EV>
__device__ __forceinline__ void sample_env_body(EV &E, const float *__restrict__ eps, int t,
                                                const mhppo_rollout_bufs &B) {
  constexpr int V = EV::VAR;
  const Cfg &c = E.c;
  const int e = E.e;
  const ObsLayout L = obs_layout(c);
  const int S = E.nS(), P = E.nP(), T = B.T;
  PlainArr<double, 2 * EV::MAXAV> act;
  const float *o = B.obs + (size_t)e * L.obs_dim;
  // One pedestrian and a compile-time S that is a multiple of 4: this env's selected
  // feature rows are feat_c[e][0..S)[0] = S*13 contiguous floats on both sides, 16-B
  // aligned (S*52 B per env), copied as float4s.
  // With one pedestrian the selected feature row of every slot is THE row, so obs_c[t] is
  // feat_c verbatim: the host points feat_c at obs_c[t] for the policy step (rollout.py
  // collect) and nothing is copied here.  Otherwise each slot's selected row is copied.
  const bool feat_in_place = B.feat_c == B.obs_c + (size_t)t * c.N * S * NF_C && P == 1;
  // compile-time S multiple of 4: the step's act/logp/rew/ep_min records go out as vectors (the
  // identity record layout; the compact one stores each present segment's record at its index)
  constexpr bool REC_VEC = EV::CNS > 0 && EV::CNS % 4 == 0;
  // the compact layout on a full wave of the register-view step: records staged per wave (RecStage)
  constexpr bool STAGE = V == V_SCALABLE && REC_VEC;
  const int32_t *rec_of = rec_map<V>(B);
  const bool vec = REC_VEC && !rec_of;
  const int lane = threadIdx.x & 63;
  const int e0 = __builtin_amdgcn_readfirstlane(e - lane);
  const bool staged = STAGE && rec_of && e0 + 64 <= c.N;
  int R0 = 0, K = 0;
  if (staged) {  // the wave's record run (uniform loads, issued with the other inputs)
    R0 = rec_of[(size_t)c.N * S + e0];
    K = rec_of[(size_t)c.N * S + e0 + 64] - R0;
  }
  // this env's records: its present slots (exist, set by mhppo_rollout_begin) in slot order from
  // the env's first record (one prefix load and the S exist bytes, not S rank loads)
  int64_t rbase = 0;
  uint32_t emask = 0;
  if (rec_of) {
    rbase = rec_of[(size_t)c.N * S + e];
    MHPPO_UNROLL
    for (int i = 0; i < S; i++) emask |= (uint32_t)(B.exist[(size_t)e * S + i] != 0) << i;
  }
  float av[REC_VEC ? EV::CNS : 1], lv[REC_VEC ? EV::CNS : 1];
  int64_t rix[EV::CNS > 0 ? EV::CNS : EV::MAXAV];  // this step's record of each slot (-1: none)
  MHPPO_UNROLL
  for (int i = 0; i < S; i++) {
    size_t row0 = ((size_t)e * S + i) * P;
    float loc = 2.0f;  // torch.tensor(car_b[1,0]) (:435)
    int sel = 0;
    MHPPO_UNROLL
    for (int p = 0; p < P; p++) {
      // scalable `if exist:` gate (:439) on the observation's exist field; the register view
      // reads the same flag from its state (pedestrian existence never changes in a step, and
      // get_data writes exactly that flag there), not a 4-B gather of the obs row
      if constexpr (V == V_SCALABLE) {
        if (EV::CNP > 0 ? !(E.pflag(p) & F_EXIST) : o[L.ped_off + p * 9 + 7] == 0.0f) continue;
      }
      float out = B.out_c[row0 + p];
      loc = t_minimum(loc, out);
      if (out == loc) sel = p;
    }
    if (loc != loc && B.status) atomicOr(B.status, 2u);  // MultivariateNormal raises on a NaN loc
    float z = eps[(size_t)e * S + i];
    float a = mvn_sample(loc, z);
    rix[i] = !rec_of ? (int64_t)e * S + i
                       : (((emask >> i) & 1u) ? rbase + __builtin_popcount(emask & ((1u << i) - 1u)) : -1);
    const int64_t bt = (int64_t)t * c.N * S + rix[i];  // time-major records [T][N S]
    if (REC_VEC && (vec || staged)) {
      av[i] = a;
      lv[i] = mvn_logp(a, loc);
    } else if (rix[i] >= 0) {
      B.act[bt] = a;
      B.logp[bt] = mvn_logp(a, loc);
    }
    if (!feat_in_place && rix[i] >= 0) {
      const float *fs = B.feat_c + (row0 + sel) * NF_C;
      float *fo = B.obs_c + bt * NF_C;
#pragma unroll
      for (int k = 0; k < NF_C; k++) fo[k] = fs[k];
    }
    act[i] = (double)a;
    // closest_ped_d starts at pedestrian 0 and only moves to another one: with one (compile-time)
    // pedestrian it is 0, and the a_d gather below does not wait on the closest[] load
    const int cp = EV::CNP == 1 ? 0 : B.closest[(size_t)e * S + i];
    act[S + i] = (double)(2 * B.a_d[row0 + cp] - 1);  // action_d_light (:423-424)
  }
  if (REC_VEC && vec) {  // this env's S records of step t are contiguous and 16-B aligned
    const size_t b0 = ((size_t)t * c.N + e) * S;
#pragma unroll
    for (int q = 0; q < (REC_VEC ? EV::CNS / 4 : 0); q++) {
      reinterpret_cast<float4 *>(B.act + b0)[q] = make_float4(av[4 * q], av[4 * q + 1], av[4 * q + 2], av[4 * q + 3]);
      reinterpret_cast<float4 *>(B.logp + b0)[q] = make_float4(lv[4 * q], lv[4 * q + 1], lv[4 * q + 2], lv[4 * q + 3]);
    }
  }
  // the episodic minima are read with the other inputs, not behind the env step's stores
  // (which the compiler may not reorder them across): no memory round trip at the end
  PlainArr<double, EV::MAXAV> epm;
  MHPPO_UNROLL
  for (int i = 0; i < S; i++) epm[i] = B.ep_min[(size_t)e * S + i];
  MHPPO_MARK(3);
  env_step_body(E, act, B.obs, nullptr);
  MHPPO_UNROLL
  for (int i = 0; i < S; i++) {
    double m = epm[i];
    double x = E.rl[i];
    epm[i] = (m != m) ? m : ((x != x) ? x : (x < m ? x : m));  // np.minimum: NaN-propagating
  }
  if constexpr (STAGE) {
    if (staged) {
      RecStage<EV::CNS> *st = rec_stage_wave<EV::CNS>();
      MHPPO_UNROLL
      for (int i = 0; i < S; i++) {
        if (rix[i] >= 0) {
          const int o = (int)(rix[i] - R0);
          st->act[o] = av[i];
          st->logp[o] = lv[i];
          st->rew[o] = E.rw[i];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int64_t base = (int64_t)t * c.N * S + R0;
      for (int j = lane; j < K; j += 64) {
        B.act[base + j] = st->act[j];
        B.logp[base + j] = st->logp[j];
        B.rew[base + j] = st->rew[j];
      }
#pragma unroll
      for (int q = 0; q < EV::CNS / 2; q++)
        reinterpret_cast<double2 *>(B.ep_min + (size_t)e * S)[q] = make_double2(epm[2 * q], epm[2 * q + 1]);
      MHPPO_MARK(10);
      MHPPO_MARK_FLUSH();
      return;
    }
  }
  if (REC_VEC && vec) {
    const size_t b0 = ((size_t)t * c.N + e) * S;
#pragma unroll
    for (int q = 0; q < (REC_VEC ? EV::CNS / 2 : 0); q++) {
      reinterpret_cast<double2 *>(B.rew + b0)[q] = make_double2(E.rw[2 * q], E.rw[2 * q + 1]);
      reinterpret_cast<double2 *>(B.ep_min + (size_t)e * S)[q] = make_double2(epm[2 * q], epm[2 * q + 1]);
    }
  } else {
    MHPPO_UNROLL
    for (int i = 0; i < S; i++) {
      if (rix[i] >= 0) B.rew[(int64_t)t * c.N * S + rix[i]] = E.rw[i];
      B.ep_min[(size_t)e * S + i] = epm[i];
    }
  }
  MHPPO_MARK(10);
  MHPPO_MARK_FLUSH();
}

template <int V>
__global__ void __launch_bounds__(TPB)
    k_sample_env(Cfg c, Bufs eb, const float *eps, int t, mhppo_rollout_bufs B, int e_lo, int e_hi) {
  int e = e_lo + blockIdx.x * TPB + threadIdx.x;
  mt_refill_wave<TPB / 64>(eb, c.N, e, e < e_hi);
  if (e >= e_hi) return;
  Env<V> E(c, eb, e);
  sample_env_body(E, eps, t, B);
}

// No MT refill in the register-view step kernel: the episode's reset kernel regenerated every stale block
// (see k_policy_mfma), and a block exhausted twice within one episode is twisted in-lane by RngT
#ifdef MHPPO_WAVE_TIMES
// A/B builds only (tools/env_waves.py): each wave's shader-clock start / end of the last launch
__device__ unsigned long long g_wave_times[2 * 8192];
#endif
template <int V, int NC, int NAV, int NP>
__global__ void __launch_bounds__(TPB)
    k_sample_env_r(Cfg c, Bufs eb, const float *eps, int t, mhppo_rollout_bufs B, int e_lo, int e_hi) {
  // envs [e_lo, e_hi) (e_lo a multiple of 64: the observation rows leave as whole wave blocks)
  const int e = e_lo + blockIdx.x * TPB + threadIdx.x;
#ifdef MHPPO_WAVE_TIMES
  const unsigned long long wt0 = __builtin_amdgcn_s_memtime();
#endif
  MHPPO_MARK(0);
  MHPPO_MARK(1);
  if (e >= e_hi) return;
  EnvR<V, NC, NAV, NP> E(c, eb, e);
  MHPPO_MARK(2);
  sample_env_body(E, eps, t, B);
#ifdef MHPPO_WAVE_TIMES
  __builtin_amdgcn_s_waitcnt(0);  // the wave's stores issued: it ends here
  const unsigned long long wt1 = __builtin_amdgcn_s_memtime();
  const int wv = e >> 6;
  if ((e & 63) == 0 && wv < 8192) {
    g_wave_times[2 * wv] = wt0;
    g_wave_times[2 * wv + 1] = wt1;
  }
#endif
}

// -------------------------------------------------------------- evaluation
// Env_rollout.iterations (:152-252; the routine Algo_PPO.evaluate runs), one lane per env
// and step: deterministic choice (argmax) when a decision is due, mean actions with the
// left-lane override and the (10 - V)/dt cap, the flat-index light quirk, env step,
// episodic min, re-decision test and saves.  Weights of the three heads in LDS.
template <int V>
__global__ void __launch_bounds__(TPB) k_eval_step(Cfg c, Bufs eb, mhppo_mlp mc, mhppo_mlp mw, mhppo_mlp md,
                                                   int t, mhppo_eval_bufs E) {
  extern __shared__ float lds[];
  const int szc = mlp_size(NF_C, 1), dc = choice_dim(c), szd = mlp_size(dc, 2);
  float *Wc = lds, *Ww = lds + szc, *Wd = lds + 2 * szc;
  for (int i = threadIdx.x; i < szc; i += blockDim.x) {
    Wc[i] = mc.packed[i];
    Ww[i] = mw.packed[i];
  }
  for (int i = threadIdx.x; i < szd; i += blockDim.x) Wd[i] = md.packed[i];
  __syncthreads();
  const int e = blockIdx.x * TPB + threadIdx.x;
  mt_refill_wave<TPB / 64>(eb, c.N, e, e < c.N);
  if (e >= c.N) return;
  const ObsLayout L = obs_layout(c);
  const int S = c.nS, P = c.P, N = c.N;
  float *o = E.obs + (size_t)e * L.obs_dim;
  int32_t *ad = E.a_d + (size_t)e * S * P;
  double *epm = E.ep_min + (size_t)e * S;
  if (t == 0 || E.trig[e]) {  // need_new_d (:175-188)
    for (int i = 0; i < S; i++) epm[i] = 0.0;
    for (int i = 0; i < S; i++)
      for (int p = 0; p < P; p++) {
        float fd[2 + 6 * (MAXS - 1) + 10], pr[2];
        obs_car_ped_d(o, L, i, p, fd);
        mlp_forward<0, 2>(Wd, dc, fd, pr);
        float p0, p1;
        softmax_pair<LibmRollout>(pr[0], pr[1], p0, p1);
        ad[i * P + p] = (p1 > p0) ? 1 : 0;  // torch.argmax: first maximum
      }
  }
  const size_t te = (size_t)t * N + e;
  if (E.obs_hist) {  // a NULL history skips its stores (include/mhppo.h mhppo_eval_step)
    float *oh = E.obs_hist + te * L.obs_dim;
    for (int k = 0; k < L.obs_dim; k++) oh[k] = o[k];
  }
  double act[2 * MAXS], rw[MAXS], rl[MAXS];
  for (int i = 0; i < S; i++) {
    double a = c.b10;  // np.array(car_b[1,0]) (:193)
    for (int p = 0; p < P; p++) {
      float f[NF_C];
      obs_car_ped(o, L, i, p, f);
      double cand;
      if (f[7] != 0.0f) {  // left the lane: speed-limit tracking, clamped (:196-197)
        double x = (10.0 - (double)f[0]) / c.dt;
        double m = (c.b10 < x) ? c.b10 : x;
        cand = (c.b00 > m) ? c.b00 : m;
      } else {
        const bool wait = (2 * ad[i * P + p] - 1) > 0;
        float out;
        mlp_forward<NF_C, 1>(wait ? Ww : Wc, NF_C, f, &out);
        const mhppo_mlp &m = wait ? mw : mc;
        cand = (double)finish_cont<LibmRollout>(out, m.mean, m.std);
      }
      if (cand < a) a = cand;  // Python min keeps the first on ties (:205-206)
      double lim = (10.0 - (double)f[0]) / c.dt;
      if (lim < a) a = lim;
    }
    act[i] = a;
    if (E.acts) E.acts[te * S + i] = (float)a;
  }
  for (int i = 0; i < S; i++) act[S + i] = (double)(2 * ad[i] - 1);  // action_d_light: flat index (:188, :210)
  const float prev1 = o[L.env_off + 1];
  env_step_one<V>(c, eb, e, act, E.obs, rw, rl, E.saved + (size_t)t * N);  // writes done into saved[t][e]
  const uint8_t done = E.saved[te];
  for (int i = 0; i < S; i++) {
    if (E.rews_c) E.rews_c[te * S + i] = (float)rw[i];
    double m = epm[i], x = rl[i];
    epm[i] = (m != m) ? m : ((x != x) ? x : (x < m ? x : m));  // np.minimum
  }
  const float cur1 = o[L.env_off + 1];
  const uint8_t trig = L.scalable ? (cur1 != (float)P) : (cur1 != prev1);  // (:218-220)
  const uint8_t saved = trig || done;
  E.saved[te] = saved;
  E.trig[e] = trig;
  if (saved) {  // (:224-229)
    if (E.rews_d)
      for (int i = 0; i < S; i++) E.rews_d[te * S + i] = (float)epm[i];
    if (E.waiting)
      for (int p = 0; p < P; p++) E.waiting[te * P + p] = (float)eb.ped[sidx(P_NF * P, P_WT * P + p, e)];
  }
}

__global__ void __launch_bounds__(TPB) k_fill_f64(double *p, size_t n, double v) {
  size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i < n) p[i] = v;
}

}  // namespace
