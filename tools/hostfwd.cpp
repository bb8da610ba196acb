// hostfwd.cpp — the batched head forward and the PPO diagnostics' per-row terms on the CPU, from
// the device source: mlp_forward (csrc/rollout_dev.h), the heads' per-row arithmetic of
// csrc/ppo_heads.h, the term functions of csrc/mlp_infer_terms.h, the very code the kernels run, and
// the scalars of csrc/ppo_math.h (MVN sample / log-prob, surrogates, torch.minimum, the Philox
// draws).  The CPU reference of tests/test_infer_host.py and tests/test_infer_gpu.py; the code under
// test of tests/test_rollout_math.py, tests/test_noise_host.py and tests/test_ppo_heads_host.py.
// Built with -ffp-contract=off: the fmaf chains are exact.
// Build: make -C tools   ->  tools/libhostfwd.so (ctypes, tools/hostfwd.py)
#include <stdint.h>

#include "../mh-ppo_amd/csrc/mlp_infer_terms.h"

using namespace mhppo;
using namespace mhppo::infer;

namespace {
bool bad_net(int kind, int n_in) { return kind < 0 || kind > 2 || n_in < 1 || n_in > N_IN_MAX; }
}  // namespace

extern "C" {
// out: [M] (kind 0: V, kind 1: mu) or [M, 2] (kind 2: probs)
int hf_forward(int kind, int n_in, const float *W, float mean, float std, const float *X, int64_t M, float *out) {
  if (bad_net(kind, n_in)) return -1;
  for (int64_t r = 0; r < M; r++) {
    const float *x = X + r * n_in;
    if (kind == 2) {
      float z[2];
      mlp_forward<0, 2>(W, n_in, x, z);
      softmax_pair<LibmRollout>(z[0], z[1], out[2 * r], out[2 * r + 1]);
    } else {
      float z;
      mlp_forward<0, 1>(W, n_in, x, &z);
      out[r] = kind == 1 ? finish_cont<LibmRollout>(z, mean, std) : z;
    }
  }
  return 0;
}

// Per row: d [M], terms [M, MHPPO_DIAG_N], logp_new [M] (the actor's log-probability of act).
// akind 1: act float32 [M]; akind 2: act int32 [M].
int hf_diag_rows(int akind, int n_in, const float *Wa, float mean, float std, const float *Wc, const float *X,
                 int64_t M, const void *act, const float *logp_old, const float *ret, double *d, double *terms,
                 float *logp_new) {
  if (bad_net(akind, n_in) || akind == 0) return -1;
  for (int64_t r = 0; r < M; r++) {
    const float *x = X + r * n_in;
    float za[2] = {0.0f, 0.0f}, vc;
    if (akind == 2) mlp_forward<0, 2>(Wa, n_in, x, za);
    else mlp_forward<0, 1>(Wa, n_in, x, za);
    mlp_forward<0, 1>(Wc, n_in, x, &vc);
    const float act_f = akind == 1 ? static_cast<const float *>(act)[r] : 0.0f;
    const int act_i = akind == 2 ? static_cast<const int32_t *>(act)[r] : 0;
    d[r] = diag_row(akind, za, mean, std, vc, act_f, act_i, logp_old[r], ret[r], terms + r * MHPPO_DIAG_N,
                    logp_new + r);
  }
  return 0;
}

// MVN(mu, 0.5).log_prob(act) as the rollout records it (ppo_math.h mvn_logp)
void hf_mvn_logp(const float *act, const float *mu, int64_t M, float *out) {
  for (int64_t r = 0; r < M; r++) out[r] = mvn_logp(act[r], mu[r]);
}

// The rest of ppo_math.h's scalars, element by element (tests/test_rollout_math.py,
// tests/test_noise_host.py)
void hf_mvn_sample(const float *loc, const float *eps, int64_t M, float *out) {
  for (int64_t r = 0; r < M; r++) out[r] = mvn_sample(loc[r], eps[r]);
}
void hf_surr_and_grad(const double *r, const double *A, int64_t M, double *f, double *dfdr) {
  for (int64_t i = 0; i < M; i++) f[i] = surr_and_grad(r[i], A[i], dfdr[i]);
}
void hf_surr_and_grad_fd(const float *r, const double *d, const float *A, int64_t M, float *f, float *dfdr) {
  for (int64_t i = 0; i < M; i++) f[i] = surr_and_grad_fd(r[i], d[i], A[i], dfdr[i]);
}
void hf_t_minimum(const float *a, const float *b, int64_t M, float *out) {
  for (int64_t i = 0; i < M; i++) out[i] = t_minimum(a[i], b[i]);
}
// draws ctr0 .. ctr0 + n - 1 (mod 2^64) under `seed`; words: uint32 [n, 4]
void hf_philox_words(uint64_t seed, uint64_t ctr0, int64_t n, uint32_t *words) {
  for (int64_t i = 0; i < n; i++) philox_words(seed, ctr0 + (uint64_t)i, words + 4 * i);
}
void hf_philox_uniform(uint64_t seed, uint64_t ctr0, int64_t n, float *out) {
  for (int64_t i = 0; i < n; i++) out[i] = philox_draw(seed, ctr0 + (uint64_t)i, false);
}
void hf_philox_normal(uint64_t seed, uint64_t ctr0, int64_t n, float *out) {
  for (int64_t i = 0; i < n; i++) out[i] = philox_draw(seed, ctr0 + (uint64_t)i, true);
}

// ---- csrc/ppo_heads.h, element by element (tests/test_ppo_heads_host.py).  update != 0: the
// LibmUpdate flavour (here the host's libm); 0: LibmRollout (the glibc restatements).
void hf_finish_cont(int update, const float *z, float mean, float std, int64_t M, float *out, float *t) {
  for (int64_t i = 0; i < M; i++)
    out[i] = update ? finish_cont<LibmUpdate>(z[i], mean, std, t[i]) : finish_cont<LibmRollout>(z[i], mean, std, t[i]);
}
void hf_softmax_pair(int update, const float *z, int64_t M, float *p) {  // z, p: [M, 2]
  for (int64_t i = 0; i < M; i++) {
    if (update) softmax_pair<LibmUpdate>(z[2 * i], z[2 * i + 1], p[2 * i], p[2 * i + 1]);
    else softmax_pair<LibmRollout>(z[2 * i], z[2 * i + 1], p[2 * i], p[2 * i + 1]);
  }
}
void hf_cat_normalise(const float *p, int64_t M, float *pn, float *sp) {  // p, pn: [M, 2]
  for (int64_t i = 0; i < M; i++) {
    float n[2];
    sp[i] = cat_normalise(p[2 * i], p[2 * i + 1], n);
    pn[2 * i] = n[0];
    pn[2 * i + 1] = n[1];
  }
}
void hf_cat_clamp(const float *pn, int64_t M, float *out) {
  for (int64_t i = 0; i < M; i++) out[i] = cat_clamp(pn[i]);
}
void hf_adv_moments(const double *stats, double m_global, float *mean_std) {
  adv_moments(stats, m_global, mean_std[0], mean_std[1]);
}
void hf_adv_normalised(const float *a, float meanf, float stdf, int64_t M, float *out) {
  for (int64_t i = 0; i < M; i++) out[i] = adv_normalised(a[i], meanf, stdf);
}
void hf_cont_logp_x(const float *act, const float *mu, int64_t M, float *lp, float *x) {
  for (int64_t i = 0; i < M; i++) lp[i] = cont_logp_x(act[i], mu[i], x[i]);
}
void hf_choice_term(const float *pn, const double *old, const double *A, const double *w, double inv_m2, int64_t M,
                    double *fk, double *dlp) {
  for (int64_t i = 0; i < M; i++) dlp[i] = choice_term(pn[i], old[i], A[i], w[i], inv_m2, fk[i]);
}
// The continuous actor's row as the train kernels chain it: y -> mu -> log-prob -> surrogate -> dL/dy.
// fd != 0: the split-precision kernel's float32 ratio with the float64 clip decision (surr_and_grad_fd).
void hf_cont_row(int fd, const float *y, float mean, float std, const float *act, const float *lp_old, const float *A,
                 double inv_m, int64_t M, double *f, float *dy) {
  for (int64_t i = 0; i < M; i++) {
    float t, x, dmu;
    const float mu = finish_cont<LibmUpdate>(y[i], mean, std, t);
    const float lp = cont_logp_x(act[i], mu, x);
    if (fd) {
      const float r = expf(lp - lp_old[i]);
      float dfdr;
      f[i] = (double)surr_and_grad_fd(r, (double)lp - (double)lp_old[i], A[i], dfdr);
      dmu = cont_dmu(inv_m, dfdr, r, x);
    } else {
      const double r = exp((double)lp - (double)lp_old[i]);
      double dfdr;
      f[i] = surr_and_grad(r, (double)A[i], dfdr);
      dmu = cont_dmu(inv_m, dfdr, r, x);
    }
    dy[i] = (dmu * std) * (1.0f - t * t);
  }
}
// The choice actor's row: y [M, 2] -> p -> pn -> the two actions' terms with weights w [M, 2] -> dL/dy [M, 2];
// f [M]: sum_k w_k f_k.  skip_zero != 0: a zero weight's term is left out (the train kernels), else added.
void hf_choice_row(const float *y, const float *lp_old, const float *A, const double *w, double inv_m2, int skip_zero,
                   int64_t M, double *f, float *dy) {
  for (int64_t i = 0; i < M; i++) {
    float p[2], pn[2];
    softmax_pair<LibmUpdate>(y[2 * i], y[2 * i + 1], p[0], p[1]);
    const float sp = cat_normalise(p[0], p[1], pn);
    double dlp[2], g0, g1, fs = 0.0;
    for (int k = 0; k < 2; k++) {
      double fk;
      dlp[k] = choice_term(pn[k], (double)lp_old[i], (double)A[i], w[2 * i + k], inv_m2, fk);
      if (!skip_zero || w[2 * i + k] != 0.0) fs += w[2 * i + k] * fk;
    }
    f[i] = fs;
    cat_grad_p(dlp, pn, sp, g0, g1);
    softmax_jacobian(p, g0, g1, dy[2 * i], dy[2 * i + 1]);
  }
}

int hf_diag_n(void) { return MHPPO_DIAG_N; }
}
