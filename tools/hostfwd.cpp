// hostfwd.cpp — the batched head forward and the PPO diagnostics' per-row terms on the CPU, from
// the device source: mlp_forward (csrc/rollout_dev.h) and the host+device finishes / term
// functions of csrc/mlp_infer_terms.h, the very code mlp_infer.hip runs, and the scalars of
// csrc/ppo_math.h (MVN sample / log-prob, surrogates, torch.minimum, the Philox draws).  The CPU
// reference of tests/test_infer_host.py and tests/test_infer_gpu.py; the code under test of
// tests/test_rollout_math.py and tests/test_noise_host.py.  Built with -ffp-contract=off: the fmaf
// chains are exact.
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
      finish_choice(z[0], z[1], out[2 * r], out[2 * r + 1]);
    } else {
      float z;
      mlp_forward<0, 1>(W, n_in, x, &z);
      out[r] = kind == 1 ? finish_cont(z, mean, std) : z;
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

int hf_diag_n(void) { return MHPPO_DIAG_N; }
}
