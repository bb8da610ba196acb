// eval_stats_terms.h — the streaming evaluation statistics' per-row arithmetic (host+device:
// eval_stats.hip runs it on the GPU, one lane per env; tools/hoststats.cpp compiles this very
// source for the CPU reference).
//
// The specification is mhppo/stats.py get_average (Coop-MH-PPO-scalable.py:1550-1675), line for
// line, over TRUE episodes (rows 0 .. T-1 of one env; pairs k = 0 .. T-2, span T-1) instead of
// maximal runs of equal crosswalk width: comparisons, differences, sy*dir, (sc - maxsx) - 25,
// (25 - sc)/vc and the could_stop test in float32; the waiting time W[n] as n repeated float64
// additions of 0.3; leave times k * 0.3 in float64 (the last matching pair; (T-1) * 0.3 when that
// k is 0 or there is none); fci / fcn cast to float32 before their float32 difference and maxima
// (NaN-propagating, as torch.max).  Every sum is a float64 sum of the float32 (waiting times:
// float64) terms get_average hands to its torch / numpy reductions; counts are integer-valued
// float64 (exact below 2^53).  Build without contraction (-ffp-contract=off), as every unit here.
#pragma once
#include "../../include/mhppo.h"
#include "env_dev.h"

namespace mhppo {
namespace evs {

constexpr double DT_STEP = 0.3;  // get_average's dt_step

// Observation columns get_average reads (split_states): car rows of cw from 0, env block, ped rows of 9.
struct Layout {
  int cw, env_off, ped_off, P, nc, obs_dim;  // nc = nb_car: the cars get_average loops over
};

// false: a layout get_average is not defined for (the 4cars drivers' car|car_follow|env|ped), or
// more cars than car slots
MHPPO_HD inline bool layout(int variant, int slots, int nb_car, int P, int obs_dim, Layout &L) {
  if (variant != V_COOP && variant != V_SCALABLE && variant != V_NAIF && variant != V_STOP) return false;
  if (nb_car < 1 || nb_car > slots || P < 1) return false;
  L.cw = variant == V_SCALABLE ? 7 : 6;
  L.env_off = L.cw * slots;
  L.ped_off = L.env_off + (variant == V_SCALABLE ? 4 : 3);
  L.P = P;
  L.nc = nb_car;
  L.obs_dim = obs_dim;
  return L.ped_off + 9 * P <= obs_dim;
}

// Per-env state, every field a column of N (field f of env e at [f * N + e]): float64 accumulators
// acc[MHPPO_EVS_N], then the float32 carry (the previous row's fields the pair tests need and the
// episode's row-0 / row-1 values), then the int32 episode counters.
MHPPO_HD inline int n_f32(const Layout &L) { return 1 + 2 * L.P + 5 * L.nc; }
MHPPO_HD inline int n_i32(const Layout &L) { return 2 * L.P + L.nc; }
MHPPO_HD inline size_t state_bytes(const Layout &L, size_t N) {
  return N * (sizeof(double) * MHPPO_EVS_N + sizeof(float) * n_f32(L) + sizeof(int32_t) * n_i32(L));
}

// One env's view of the state.  ABS (the host harness): abs_[j] accumulates |term| beside acc[j].
template <bool ABS>
struct View {
  double *acc, *abs_;
  float *f;
  int32_t *i;
  size_t N, e;
  MHPPO_HD View(void *state, double *abs_sums, const Layout &L, size_t N_, size_t e_) : N(N_), e(e_) {
    acc = static_cast<double *>(state);
    f = reinterpret_cast<float *>(acc + (size_t)MHPPO_EVS_N * N);
    i = reinterpret_cast<int32_t *>(f + (size_t)n_f32(L) * N);
    abs_ = abs_sums;
  }
  MHPPO_HD void add(int j, double x) {
    acc[(size_t)j * N + e] += x;
    if (ABS) abs_[(size_t)j * N + e] += x < 0.0 ? -x : x;
  }
  MHPPO_HD void moments(int jn, int js, int jq, float x) {  // count, sum, sum of squares of a float32 term
    const double d = (double)x;
    add(jn, 1.0);
    add(js, d);
    add(jq, d * d);
  }
  MHPPO_HD float &F(int k) { return f[(size_t)k * N + e]; }
  MHPPO_HD int32_t &I(int k) { return i[(size_t)k * N + e]; }
};

// carry columns
MHPPO_HD inline int f_cross() { return 0; }
MHPPO_HD inline int f_sy(const Layout &, int p) { return 1 + p; }
MHPPO_HD inline int f_dr(const Layout &L, int p) { return 1 + L.P + p; }
MHPPO_HD inline int f_car(const Layout &L, int field, int i) { return 1 + 2 * L.P + field * L.nc + i; }
enum { FC_SC, FC_VC, FC_LIGHT, FC_L1, FC_FCN };  // previous sc / vc / light; light at row 1; (25 - sc0) / vc0
MHPPO_HD inline int i_cnt(const Layout &, int p) { return p; }           // waiting pairs so far
MHPPO_HD inline int i_lkp(const Layout &L, int p) { return L.P + p; }    // last k of the ped-leave test
MHPPO_HD inline int i_lkc(const Layout &L, int i) { return 2 * L.P + i; }  // last k of the car-leave test; bit 30: could_stop at row 0
constexpr int32_t CS_BIT = 1 << 30;

MHPPO_HD inline float absf(float x) { return x < 0.0f ? -x : x; }
// torch.max over a dimension: NaN wins
MHPPO_HD inline float max_nan(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b > a ? b : a)); }
// W[n] of get_average: n Python float additions of 0.3, left to right
MHPPO_HD inline double repeated_add(int n) {
  double acc = 0.0;
  for (int k = 0; k < n; k++) acc += DT_STEP;
  return acc;
}

// Row t (< T, T >= 2) of the env's current episode; o: its observation row.
template <bool ABS>
MHPPO_HD inline void row(const float *o, const Layout &L, int t, int T, View<ABS> &s) {
  const float *env = o + L.env_off, *ped = o + L.ped_off;
  const float cross = env[0];
  // ---- row-level moments (every row of every episode)
  {
    const float v0 = o[1], a0 = o[0], vp = absf(ped[1]);
    s.add(MHPPO_EVS_ROWS, 1.0);
    s.add(MHPPO_EVS_V0, (double)v0);
    s.add(MHPPO_EVS_V0_SQ, (double)v0 * (double)v0);
    s.add(MHPPO_EVS_ABSA0, (double)absf(a0));
    s.add(MHPPO_EVS_A0, (double)a0);
    s.add(MHPPO_EVS_A0_SQ, (double)a0 * (double)a0);
    s.add(MHPPO_EVS_ABSVP0, (double)vp);
    s.add(MHPPO_EVS_ABSVP0_SQ, (double)vp * (double)vp);
  }
  const int k = t - 1;  // the pair (t - 1, t) this row closes
  const bool last = t == T - 1;
  const double span_dt = (double)(T - 1) * DT_STEP;
  float maxsx = ped[2];
  for (int p = 1; p < L.P; p++) maxsx = max_nan(maxsx, ped[9 * p + 2]);
  float max_fci = 0.0f, max_fcn = 0.0f;  // the episode's maxima over (peds, cars), at the last row
  // ---- pedestrians
  for (int p = 0; p < L.P; p++) {
    const float sy = ped[9 * p + 3], dr = ped[9 * p + 8];
    if (t == 0) {
      s.I(i_cnt(L, p)) = 0;
      s.I(i_lkp(L, p)) = 0;
    } else {
      const float psy = s.F(f_sy(L, p)), pdr = s.F(f_dr(L, p)), pcross = s.F(f_cross());
      const bool c1 = absf(psy) == pcross && absf(sy) == cross;
      const bool c2 = absf(psy) == 0.0f && absf(sy) == 0.0f;
      const bool c3 = (psy * pdr) < pcross && (sy * dr) >= cross;
      const int add = (c1 ? 1 : 0) + (c2 ? 1 : 0);
      if (add) s.I(i_cnt(L, p)) += add;
      if (c3) s.I(i_lkp(L, p)) = k;
    }
    if (last) {
      const double wt = repeated_add(s.I(i_cnt(L, p)));
      const int lk = s.I(i_lkp(L, p));
      const double pl = lk == 0 ? span_dt : (double)lk * DT_STEP;
      const float fci = (float)pl, fcn = (float)(pl - wt);
      s.moments(MHPPO_EVS_N_PED, MHPPO_EVS_PEDT, MHPPO_EVS_PEDT_SQ, fci);
      s.add(MHPPO_EVS_WAIT, wt);
      s.add(MHPPO_EVS_WAIT_SQ, wt * wt);
      s.add(MHPPO_EVS_FC, (double)(fci - fcn));
      max_fci = p == 0 ? fci : max_nan(max_fci, fci);
      max_fcn = p == 0 ? fcn : max_nan(max_fcn, fcn);
    } else {
      s.F(f_sy(L, p)) = sy;
      s.F(f_dr(L, p)) = dr;
    }
  }
  // ---- cars
  float dec[2] = {0.0f, 0.0f};
  for (int i = 0; i < L.nc; i++) {
    const float *car = o + i * L.cw;
    const float sc = car[3], vc = car[1], li = car[4];
    if (t == 0) {
      s.F(f_car(L, FC_FCN, i)) = (25.0f - sc) / vc;
      const float brake = vc * vc / 8.0f + vc;
      s.I(i_lkc(L, i)) = ((-sc - brake) > 0.0f) ? CS_BIT : 0;
    } else {
      const float psc = s.F(f_car(L, FC_SC, i)), pvc = s.F(f_car(L, FC_VC, i));
      if (t == 1) {
        s.F(f_car(L, FC_L1, i)) = li;
        if (li < 0.0f) {  // could_stop is appended when the light at row 1 is go
          s.add(MHPPO_EVS_N_CS, 1.0);
          s.add(MHPPO_EVS_CS, (s.I(i_lkc(L, i)) & CS_BIT) ? 1.0 : 0.0);
        }
      }
      const float l1 = t == 1 ? li : s.F(f_car(L, FC_L1, i));
      const float d0 = (psc - maxsx) - 25.0f, d1 = (sc - maxsx) - 25.0f;
      const bool c4 = d0 < 0.0f && d1 >= 0.0f;
      if (c4) s.I(i_lkc(L, i)) = (s.I(i_lkc(L, i)) & CS_BIT) | k;
      if (l1 == 1.0f) {  // the yield lists: every pair of an episode whose car yields
        s.moments(MHPPO_EVS_N_YSPEED, MHPPO_EVS_YSPEED, MHPPO_EVS_YSPEED_SQ, pvc);
        if (c4) s.moments(MHPPO_EVS_N_YTIME, MHPPO_EVS_YTIME, MHPPO_EVS_YTIME_SQ, (float)((double)k * DT_STEP));
      }
    }
    if (last) {
      const int lk = s.I(i_lkc(L, i)) & ~CS_BIT;
      const double cl = lk == 0 ? span_dt : (double)lk * DT_STEP;
      const float fci = (float)cl, fcn = s.F(f_car(L, FC_FCN, i));
      s.moments(MHPPO_EVS_N_CAR, MHPPO_EVS_CART, MHPPO_EVS_CART_SQ, fci);
      s.add(MHPPO_EVS_FC, (double)(fci - fcn));
      max_fci = max_nan(max_fci, fci);
      max_fcn = max_nan(max_fcn, fcn);
      const float d = s.F(f_car(L, FC_LIGHT, i));  // decision: the light at row T - 2
      if (d == 1.0f) s.add(MHPPO_EVS_YIELD, 1.0);
      if (d == -1.0f) s.add(MHPPO_EVS_GO, 1.0);
      if (i < 2) dec[i] = d;
    } else {
      s.F(f_car(L, FC_SC, i)) = sc;
      s.F(f_car(L, FC_VC, i)) = vc;
      s.F(f_car(L, FC_LIGHT, i)) = li;
    }
  }
  if (last) {
    s.add(MHPPO_EVS_EPISODES, 1.0);
    s.add(MHPPO_EVS_IC, (double)(max_fci - max_fcn));
    if (L.nc == 2) {
      const float sum = dec[0] + dec[1];
      if (sum == 2.0f) s.add(MHPPO_EVS_SC_YY, 1.0);
      if (sum == -2.0f) s.add(MHPPO_EVS_SC_GG, 1.0);
      if (dec[0] == -1.0f && dec[1] == 1.0f) s.add(MHPPO_EVS_SC_GY, 1.0);
      if (dec[0] == 1.0f && dec[1] == -1.0f) s.add(MHPPO_EVS_SC_YG, 1.0);
    }
  } else {
    s.F(f_cross()) = cross;
  }
}

}  // namespace evs
}  // namespace mhppo
