/* mhppo.h — C-ABI of libmhppo.so, the MI355X-native hot path of MH-PPO.
 *
 * The reference is pure Python (no FFI); each entry point below replaces a
 * Python call site on the hot path.  Callers bind it
 * with ctypes (mh-ppo_amd/mhppo/_lib.py; INTEGRATION.md shows the binding a
 * maintainer of the reference would add).
 *
 * Conventions
 *  - Every function returns 0 on success or a negative MHPPO_E* code;
 *    mhppo_last_error() returns a thread-local message for the last failure.
 *  - All data pointers are DEVICE pointers owned by the caller (e.g. torch
 *    tensor data_ptr()s on the handle's device); nothing is freed across the ABI.
 *  - Calls are asynchronous on `stream` (a hipStream_t, NULL = default stream).
 *  - A handle is bound to one device and is not re-entrant.
 */
#ifndef MHPPO_H
#define MHPPO_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHPPO_OK 0
#define MHPPO_EINVAL -1   /* invalid configuration / argument */
#define MHPPO_EHIP -2     /* HIP runtime error */
#define MHPPO_ENOMEM -3   /* device allocation failed */
#define MHPPO_ENAN -4     /* NaN policy output: the reference raises ValueError from torch.distributions'
                             argument validation (Categorical probs / MultivariateNormal loc) */

/* Env variants = the reference gym ids (Environments/__init__.py:3-42). */
#define MHPPO_COOP 0      /* Crosswalk_hybrid_multi_coop-v0          Env_hybrid_multi_coop.py:625 */
#define MHPPO_4CARS 1     /* Crosswalk_hybrid_multi_coop_4cars-v0    Env_hybrid_multi_coop_4cars.py:667 */
#define MHPPO_SCALABLE 2  /* Crosswalk_hybrid_multi_coop_scalable-v0 Env_hybrid_multi_coop_scalable.py:668 */
#define MHPPO_NAIF 3      /* Crosswalk_hybrid_multi_naif-v0          Env_hybrid_multi_naif.py:616 */
#define MHPPO_4CARS2 4    /* Crosswalk_hybrid_multi_coop_4cars2-v0   Env_hybrid_multi_coop_4cars2.py:683
                             (env only: actions [AV acc, follower acc, AV light, follower light]) */
#define MHPPO_STOP 5      /* Crosswalk_hybrid_multi_stop-v0          Env_hybrid_multi_stop.py:634 */
/* mhppo_env_cfg.flags */
#define MHPPO_FIX_SCALABLE_LANES 1 /* scalable: build slot i's car with i (lane i//2, follower 20 m behind
                                      when i is odd) instead of i//2 (lane (i//2)//2, :900-906, :537, :576) */
#define MHPPO_GENERIC_STEP 2       /* not a semantic flag: always run the step on the generic in-HBM env view
                                      (the register view serves the shapes it is compiled for; tests compare both) */

typedef struct mhppo_env_cfg {
    int32_t variant;      /* MHPPO_* */
    int32_t n_envs;       /* N: envs on this handle (this rank's shard) */
    int32_t nb_car, nb_ped, nb_lines;
    int32_t max_episode;  /* 80 in every reference driver */
    int32_t sin_model;    /* simulation == "sin" */
    int32_t flags;        /* opt-in bug fixes, 0 = the reference's behaviour */
    double dt;            /* 0.3 */
    double car_b[4];      /* row-major [[acc_min, v],[acc_max, v]] */
    double ped_b[8];      /* row-major [2][4] */
    double cross_b[2];
    uint64_t seed_base;   /* env e draws from random.seed(seed_base + env_id_offset + e) */
    uint64_t env_id_offset;
} mhppo_env_cfg;

typedef struct mhppo_env mhppo_env;

/* Replaces gym.make(id, car_b=..., ...) -> Crosswalk_*.__init__ (Env_hybrid_multi_coop.py:637-692)
 * plus the module-import `random.seed(10)` (:10), per env: seeds N CPython
 * MT19937 streams on the device. */
int mhppo_env_create(const mhppo_env_cfg *cfg, int device, mhppo_env **out);
void mhppo_env_destroy(mhppo_env *env);

/* Geometry of the flat observation (gym-sorted keys car|car_follow|env|ped) and slots. */
int mhppo_env_obs_dim(const mhppo_env *env);
int mhppo_env_slots(const mhppo_env *env);   /* S: action slots per env (actions are [N, 2S]) */
int mhppo_env_reward_slots(const mhppo_env *env); /* reward/reward_light width: S, except 4cars2 = nb_car
                                                     (its PPO-driven followers earn none, :836-847) */

/* Checkpoint/resume (the reference saves only weights, :985-1001):
 * the env's whole device state — every field of every env plus its CPython MT19937
 * stream (624 words + cursor) — as one opaque blob of mhppo_env_state_bytes bytes.
 * export copies it to `dst`, import restores it from `src` (host or device memory,
 * stream-ordered); a blob is valid only for a handle created with the same config. */
int64_t mhppo_env_state_bytes(const mhppo_env *env);
int mhppo_env_export(const mhppo_env *env, void *dst, void *stream);
int mhppo_env_import(mhppo_env *env, const void *src, void *stream);

/* Replaces Crosswalk_*.reset() (Env_hybrid_multi_coop.py:838-893; 4cars :850-911;
 * scalable :884-946).  obs: float32 [N, obs_dim] or NULL. */
int mhppo_env_reset(mhppo_env *env, float *obs, void *stream);

/* Replaces Env_rollout.choix_test (Coop-MH-PPO-scalable.py:629-633) + env.get_state(), the
 * scripted scenario evaluate(n, choix=True) plays after every reset (:170-172): cross 3,
 * pedestrians rebuilt with pedestrian 0 crossing from (0, -1) at 1.25 m/s, cars 0/1 at -45 /
 * -22 m on lanes 0 / 1.  Scalable env only (MHPPO_EINVAL otherwise).  obs: float32
 * [N, obs_dim] or NULL. */
int mhppo_env_choix_test(mhppo_env *env, float *obs, void *stream);

/* Replaces Crosswalk_*.step(actions) (Env_hybrid_multi_coop.py:745-832; 4cars :783-844;
 * scalable :789-878).  actions: float64 [N, 2S] = [acc_0..acc_{S-1}, light_0..light_{S-1}];
 * obs float32 [N, obs_dim] (nullable); rewards, reward_light float64 [N, S];
 * done uint8 [N]. */
int mhppo_env_step(mhppo_env *env, const double *actions, float *obs, double *rewards,
                   double *reward_light, uint8_t *done, void *stream);

/* Read back the per-env scalar/attribute view the reference drivers touch
 * (env.cross, ped_traffic, car_traffic, cars[i].exist, pedestrian[j].waiting_time,
 * internal flags): out float64 [N, mhppo_env_state_dim() = 21P + 8 car slots + 4], laid out
 * [per ped 20][per car slot 8][cross, time, ped_traffic, car_traffic][per ped exist]. */
int mhppo_env_state_dim(const mhppo_env *env);
int mhppo_env_get_state(mhppo_env *env, double *out, void *stream);
/* Per-env event counters since the env's last reset (SURVEY §5 Metrics): the reference's only
 * run-time diagnostics are five prints inside pedestrian.detection; each one the reference would
 * print increments the env's counter instead (no device printf).  out uint32 [N, MHPPO_EV_N]. */
#define MHPPO_EV_ACCIDENT 0  /* "Accident! : "                scalable :186, 4cars :293, coop :185 */
#define MHPPO_EV_POSSIBLE 1  /* "Possible accident! "         scalable :200, 4cars :307, coop :199 */
#define MHPPO_EV_SMALL 2     /* "Small mistake - priority ? " scalable :222, 4cars :320, coop :221 */
#define MHPPO_EV_NOTWAIT 3   /* "Pedestrian is not waiting "  scalable :227, 4cars :325, coop :226
                                (once per pedestrian; naif :224 every time) */
#define MHPPO_EV_GREEN 4     /* "Mauvais signal vert "        scalable :236, 4cars :334, coop :235 */
#define MHPPO_EV_N 5
int mhppo_env_events(mhppo_env *env, uint32_t *out, void *stream);
/* RNG cursor: mt uint32 [N, 624], mti int32 [N] (device). */
int mhppo_env_get_rng(mhppo_env *env, uint32_t *mt, int32_t *mti, void *stream);

/* ---- rollout collector (Env_rollout.iterations_rand, Coop-MH-PPO-scalable.py:357-517) ---- */

/* One Model_PPO MLP (Coop-MH-PPO-scalable.py:42-93), in -> 32 -> 64 -> 32 -> out, ReLU,
 * packed contiguously in torch layout: W1[32][in] b1[32] W2[64][32] b2[64] W3[32][64]
 * b3[32] W4[out][32] b4[out] (float32, device).  kind: 0 linear (critic), 1 tanh*std+mean
 * (continuous actor), 2 pairwise softmax (choice actor). */
typedef struct mhppo_mlp {
    const float *packed;
    int32_t n_in, n_out, kind, reserved;
    float mean, std;
} mhppo_mlp;

/* Per-iteration rollout buffers for N envs, S slots, P peds, T steps (device, caller-owned).
 * Shapes: feat_d [N,S,P,dc] f32, probs_d [N,S,P,2] f32, a_d [N,S,P] i32, logp_d [N,S,P] f32,
 * closest [N,S] i32, feat_c [N,S,P,13] f32, out_c [N,S,P] f32, obs [N,obs_dim] f32 (current
 * observation), ep_min [N,S] f64, exist [N,S] u8, and the per-step records TIME-MAJOR (step t
 * of every env is one contiguous block): obs_c [T,N,S,13] f32, act [T,N,S] f32, logp [T,N,S]
 * f32, rew [T,N,S] f64.  The reference's episode-major batch order (:489-507) is a gather
 * of (env, slot) segments over t, see mhppo/rollout.py bucket_segments.
 * With P == 1, feat_c may point at obs_c + t*N*S*13 for step t (the selected feature row is
 * the only row, so the policy writes the record in place and sample_env copies nothing).
 * rows (int32 [N*S*P + 2]; required by the policy step, which returns MHPPO_EINVAL without it):
 * scratch for the head-sorted policy step — begin lists the (env, slot, ped) rows of the cross
 * head, then those of the wait head, counts last. */
typedef struct mhppo_rollout_bufs {
    float *feat_d, *probs_d, *logp_d;
    int32_t *a_d, *closest;
    float *feat_c, *out_c, *obs;
    float *obs_c, *act, *logp;
    double *rew, *ep_min;
    uint8_t *exist;
    int32_t *rows;
    int32_t T, flags;   /* flags: MHPPO_ROLLOUT_* */
    uint32_t *status;   /* optional device word, zeroed by mhppo_rollout_begin (flags of the current
                           episode only): bit 0 = a NaN choice probability, bit 1 = a NaN continuous
                           action mean was sampled; see mhppo_rollout_check */
    int32_t parts;      /* 0/1, or P > 1: the envs split in P contiguous parts (boundaries at multiples
                           of 64 envs) whose steps run as independent chains, e.g. on P streams
                           (mhppo_rollout_policy_part / _sample_env_part); rows then needs
                           N*S*P + 2 + 2 (parts + 1) entries */
    int32_t reserved;
    int32_t *rec_of;    /* optional [N*S + N + 1] (NULL: record index = segment index): the compact
                           record layout.  mhppo_rollout_begin fills it from exist: segment s = env*S
                           + slot gets record rec_of[s] = its rank among the existing segments, or -1,
                           and rec_of[N*S + e] = the existing segments before env e (e = 0 .. N);
                           every per-step record of segment s (obs_c row, act, logp, rew) is then
                           stored at record rec_of[s] of step t (obs_c[t][rec_of[s]], ...), and none
                           for rec_of[s] = -1, so the present segments' records are contiguous and
                           absent ones cost no stores (and share no cache line with present ones
                           for mhppo_bucket_scatter, whose pos / bucket are then per record).  With
                           one pedestrian (P == 1) feat_c must be obs_c[t] (the in-place record).
                           The scalable env only (the variant whose car slots can be absent):
                           mhppo_rollout_begin returns MHPPO_EINVAL for another. */
} mhppo_rollout_bufs;
/* mhppo_rollout_bufs.flags: run the policy step on the VALU reference kernels instead of the MFMA
 * kernel (bit-identical).  Those kernels are compiled into the test build only
 * (tests/lib/libmhppo_test.so, -DMHPPO_TEST_KERNELS); the shipped library returns MHPPO_EINVAL. */
#define MHPPO_ROLLOUT_VALU_POLICY 1
#define MHPPO_ROLLOUT_VALU_UNSORTED 2 /* with _VALU_POLICY: the unsorted one-lane-per-row kernel (test build only) */

int mhppo_choice_dim(const mhppo_env *env);

/* Deterministic evaluation (Env_rollout.iterations :152-252, run by Algo_PPO.evaluate
 * :738-747).  Device buffers; per-step outputs are time-major [T][N][..]. */
typedef struct mhppo_eval_bufs {
    float *obs;       /* [N, obs_dim] current observation (in/out; mhppo_env_reset fills it) */
    int32_t *a_d;     /* [N, S, P] current choice (argmax of the choice actor) */
    uint8_t *trig;    /* [N] re-decision due at the next step */
    double *ep_min;   /* [N, S] episodic min of reward_light since the last decision */
    float *obs_hist;  /* [T, N, obs_dim] pre-step observations (batch_obs) */
    float *acts;      /* [T, N, S] continuous actions (batch_acts) */
    float *rews_c;    /* [T, N, S] step rewards (batch_rews_c) */
    float *rews_d;    /* [T, N, S] episodic reward at a save (batch_rews_d), rows with saved = 1 */
    float *waiting;   /* [T, N, P] pedestrians' waiting_time at a save, rows with saved = 1 */
    uint8_t *saved;   /* [T, N] a save happened after step t (re-decision or done) */
    int32_t T, reserved;
} mhppo_eval_bufs;

/* Step t of an evaluation episode in every env (t = 0 right after mhppo_env_reset):
 * choice argmax when a decision is due (t = 0 or the re-decision test fired), per car
 * a = min over pedestrians of the head's mean action (left-lane pedestrians: clamped
 * speed-limit tracking), capped by (10 - V)/dt; lights = 2 a_d[flat i] - 1; env step.
 * A NULL obs_hist, acts, rews_c, rews_d or waiting skips that history's stores (the streaming
 * statistics below keep none); saved [T, N] stays required: it is the step's done scratch. */
int mhppo_eval_step(mhppo_env *env, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                    const mhppo_mlp *actor_choice, int t, mhppo_eval_bufs *bufs, void *stream);

/* Episode start (:377-428): reset every env, write obs, choice features obs_car_ped_d
 * (:574-611) and closest pedestrian (:614-627), run the choice actor and draw
 * Categorical samples.  When `forced_a` (int32 [N,S,P]) is non-NULL the draws are
 * replayed from it (parity mode); otherwise u (float32 [N,S,P] uniforms) picks
 * a = (u >= p0/(p0+p1)). */
int mhppo_rollout_begin(mhppo_env *env, const mhppo_mlp *actor_choice, const float *u,
                        const int32_t *forced_a, mhppo_rollout_bufs *bufs, void *stream);

/* Step t (:430-461): obs_car_ped features for every (slot, ped) (:541-572), cross/wait
 * actor chosen by action_d (:440-445), min over pedestrians, MVN(loc, 0.5) sample from
 * eps (float32 [N,S] standard normals), env.step, episodic min of reward_light (:461). */
int mhppo_rollout_step(mhppo_env *env, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                       const float *eps, int t, mhppo_rollout_bufs *bufs, void *stream);
/* The two launches of mhppo_rollout_step, separately (for per-kernel timing):
 * policy = features + actor forward per (env, slot, ped); sample_env = per-env
 * min/sample/buffers + env.step + episodic min. */
int mhppo_rollout_policy(mhppo_env *env, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                         mhppo_rollout_bufs *bufs, void *stream);
int mhppo_rollout_sample_env(mhppo_env *env, const float *eps, int t, mhppo_rollout_bufs *bufs, void *stream);
/* The same two launches for part `part` of bufs->parts only (its envs' rows / its envs): the parts'
 * step chains are independent, so on separate streams one part's policy MFMA work fills the CUs
 * another part's latency-bound env step leaves idle.  Results are those of the whole-N calls. */
int mhppo_rollout_policy_part(mhppo_env *env, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                              mhppo_rollout_bufs *bufs, int part, void *stream);
int mhppo_rollout_sample_env_part(mhppo_env *env, const float *eps, int t, mhppo_rollout_bufs *bufs, int part,
                                  void *stream);

/* Measurement (bench.py): the next `n` env-step launches (mhppo_rollout_sample_env) of the
 * calling thread on the device current at this call carry HIP events attached to their dispatch
 * packets (hipExtLaunchKernelGGL start/stop events: the kernel's execution, not the queue's
 * event-packet gaps);
 * mhppo_kernel_timing_end synchronises them and returns the summed milliseconds and the
 * number of timed launches.  No reference counterpart. */
int mhppo_kernel_timing_begin(int n);
int mhppo_kernel_timing_end(double *ms_total, int *launches);
/* As mhppo_kernel_timing_end, but writes each timed launch's milliseconds, in launch order, to
 * ms_each[0 .. min(cap, launches)) (the per-step durations of a rollout: tools/env_steps.py). */
int mhppo_kernel_timing_end_each(float *ms_each, int cap, int *launches);

/* Status of the rollout launches queued on `stream` so far: synchronises the stream, reads
 * and clears bufs->status, and returns MHPPO_ENAN when a NaN policy output was drawn from
 * (Categorical(probs) at the episode start, :409; MultivariateNormal(loc) per step, :451:
 * where the reference's torch.distributions raise ValueError), else MHPPO_OK. */
int mhppo_rollout_check(mhppo_rollout_bufs *bufs, void *stream);

/* Philox-4x32-10 noise (perf mode): out[i] for counter (offset + i) under key `seed`. */
int mhppo_philox_normal(uint64_t seed, uint64_t offset, float *out, int64_t n, void *stream);
int mhppo_philox_uniform(uint64_t seed, uint64_t offset, float *out, int64_t n, void *stream);
/* rows x cols normals, out[r * cols + c] from counter (offset + r * stride + c): a rollout's
 * per-step noise in one launch (the same values as `rows` calls of mhppo_philox_normal). */
int mhppo_philox_normal_2d(uint64_t seed, uint64_t offset, uint64_t stride, float *out, int64_t rows,
                           int64_t cols, void *stream);

/* ---- returns / advantage / PPO losses (futur_rewards :658-684, train_model_c/_d :778-851) ---- */

/* The rollout policy heads' float transcendentals (csrc/libm_glibc.h: glibc 2.35's tanhf, expm1f,
 * expf restated so the device returns glibc's bits — the functions the reference's batch-1 CPU
 * forward calls, Model_PPO :81-89) evaluated on the float bit patterns first .. first + n - 1
 * (mod 2^32): the device side of their exhaustive pin (tests/test_libm_gpu.py).
 * fn: 0 tanhf, 1 expm1f, 2 expf.  out float [n]. */
int mhppo_libm_eval(int fn, uint64_t first, int64_t n, float *out, void *stream);

/* Segmented reverse discounted scan, G_t = r_t + gamma*G_{t+1} in float64, one segment of
 * T per row: rew float64 [B,T] -> ret float32 [B,T]. */
int mhppo_returns_scan(const double *rew, float *ret, int64_t B, int32_t T, double gamma, void *stream);
/* The same scan over time-major records: rew float64 [T,B] -> ret float32 [T,B] (segment b
 * is column b; the rollout's rew buffer is [T, N*S]). */
int mhppo_returns_scan_tm(const double *rew, float *ret, int64_t B, int32_t T, double gamma, void *stream);

/* Segment-major buckets (bucket_segments; replaces the per-episode concatenation of
 * Coop-MH-PPO-scalable.py:489-507).  Segment s < NS (= N*S records per step) with pos[s] >= 0
 * belongs to bucket bucket[s] (0 or 1) at position pos[s]: its time-major records t < T
 * (obs [.., 13] float32, act / logp / ret float32, rew float64; record t*NS + s) go to rows
 * pos[s]*T + t of dst[bucket[s]] (caller-sized: count of segments x T rows). */
typedef struct {
  float *obs, *act, *logp, *ret;
  double *rew;
} mhppo_bucket_dst;
int mhppo_bucket_scatter(const int64_t *pos, const int8_t *bucket, int64_t NS, int32_t T, const float *obs_tm,
                         const float *act_tm, const float *logp_tm, const float *ret_tm, const double *rew_tm,
                         const mhppo_bucket_dst *dst, void *stream);

/* mhppo_bucket_scatter that also adds to rew_sums[b] the float64 sum of (double)(float)rew over
 * bucket b's rows (the reward curves' sums, Algo_PPO.train :886-892): per-block partials folded in
 * a fixed order (deterministic, no atomics; the caller zeroes rew_sums, or mhppo_bucket_plan has).
 * dst[0] and dst[1] may name the same buffers (both buckets in one shared buffer: bucket[] then
 * only keys the sums).  work: mhppo_bucket_work_bytes(NS, T) bytes of device scratch, 8-byte
 * aligned. */
int mhppo_bucket_scatter_sums(const int64_t *pos, const int8_t *bucket, int64_t NS, int32_t T, const float *obs_tm,
                              const float *act_tm, const float *logp_tm, const float *ret_tm, const double *rew_tm,
                              const mhppo_bucket_dst *dst, double *rew_sums, void *work, void *stream);

/* The bucket plan (bucket_segments; Coop-MH-PPO-scalable.py:489-507): everything the bucketing
 * decides per (env, slot) segment s < NS = N*S, on the device, in three launches (per-block counts,
 * a one-block scan of them, placement: no block waits on another) before the caller's one read of
 * `info`.
 * In: a_d int32 [N, S*P] (the choice actions), closest int32 [NS] (each car's closest pedestrian),
 * exist uint8 [NS], rec_of int32 [NS] or NULL (the compact record layout: segment s's record index,
 * < 0 = none), ep_min float64 [NS], feat_d float32 [NS*P, dc], logp_d float32 [NS*P], fix_bucket,
 * status int32 [1] or NULL (the rollout's NaN-flag word, copied to info).
 * Bucket rule: only existing segments; segment s = (env n, slot i) is cross when action_d[i] <= 0,
 * action_d = 2 a_d[n] - 1 indexed by the CAR index i, or with fix_bucket by the car's
 * own closest pedestrian, a_d[s*P + closest[s]]; wait otherwise.
 * Out: pos int64 [NS] / bucket int8 [NS] as mhppo_bucket_scatter takes them (per record when
 * rec_of is given): cross segments ranked from 0 in (env, slot) order, bucket 0; wait segments
 * ranked from w0 = (n_cross + 3) / 4 * 4, bucket 1 — positions in ONE shared buffer of
 * (NS + 3) * T rows; everything else pos -1, bucket 0.
 * The choice batch, existing segments first in (env, slot) order, row k taken at
 * b = s*P + closest[s] of the k-th existing segment s: c_obs [., dc] = feat_d[b], c_act int32 =
 * a_d[b], c_logp = logp_d[b], c_ret = (float)ep_min[s]; caller-sized for NS rows, rows >= n_all
 * are not written.
 * info (device): the sizes, the status word, counts = the existing segments with c_act == 0 / == 1,
 * rew_sums[2] = the float64 sum of c_ret (per-block partials, fixed order); rew_sums[0..1] are
 * zeroed for mhppo_bucket_scatter_sums to add the cross / wait sums.
 * work: mhppo_bucket_work_bytes(NS, T) bytes of device scratch, 8-byte aligned. */
typedef struct {
  int64_t n_cross, n_wait, n_all, status;
  double counts[2];
  double rew_sums[3];
} mhppo_bucket_info;
int64_t mhppo_bucket_work_bytes(int64_t NS, int32_t T);
int mhppo_bucket_plan(int64_t N, int32_t S, int32_t P, int32_t dc, const int32_t *a_d, const int32_t *closest,
                      const uint8_t *exist, const int32_t *rec_of, const double *ep_min, const float *feat_d,
                      const float *logp_d, int32_t fix_bucket, const int32_t *status, int64_t *pos, int8_t *bucket,
                      float *c_obs, int32_t *c_act, float *c_logp, float *c_ret, mhppo_bucket_info *info,
                      void *work, void *stream);

/* Advantage statistics of A = G - V over M rows: stats float64 [2] += (sum A, sum A^2)
 * (caller zeroes it; partial sums all-reduce across ranks).  Normalisation
 * A' = (A - mean) / (std_unbiased + 1e-10) with mean/std from (stats, M_global). */
int mhppo_adv_stats(const float *ret, const float *value, int64_t M, double *stats, void *stream);
int mhppo_adv_normalize(const float *ret, const float *value, int64_t M, const double *stats,
                        double m_global, float *adv, void *stream);

/* Continuous PPO clip surrogate (:795-806): logp = MVN(mu, 0.5).log_prob(act) (float32),
 * ratio = exp(logp - logp_old) in float64, L = mean(-min(r A, clamp(r, .8, 1.2) A)).
 * dmu float32 [M] = dL/dmu with the 1/M_global factor (inv_m); loss float64 [1] += sum. */
int mhppo_ppo_cont_fwd_bwd(const float *mu, const float *act, const float *logp_old,
                           const float *adv, int64_t M, double inv_m, float *dmu,
                           double *loss, void *stream);

/* Choice PPO surrogate over the reference's M x M broadcast (:834-842) in its exact O(M)
 * form L = (1/M^2) sum_j [n0 f(r_j0, A_j) + n1 f(r_j1, A_j)], f(r,A) = -min(rA, clip(r)A),
 * r_jk = exp(log clamp(p_jk/(p_j0+p_j1)) - logp_old_j).  probs float32 [M,2] (softmax
 * outputs); counts float64 [2] = (n0, n1) global.  dprobs float32 [M,2] = dL/dprobs. */
int mhppo_ppo_choice_fwd_bwd(const float *probs, const float *logp_old, const float *adv,
                             int64_t M, const double *counts, double inv_m2, float *dprobs,
                             double *loss, void *stream);

/* Fused training pass of one Model_PPO head (n_in -> 32 -> 64 -> 32 -> n_out) on f32 MFMA:
 * forward + loss gradient + backward + weight gradient over M rows, replacing the torch
 * GEMMs/autograd of one epoch of train_model_c (:778-815) / train_model_d (:818-851).
 * kind 0 = critic (n_in <= 64, n_out 1): writes value[M]; grad = dMSE/dW;
 *          sums[0..2] += (sum (V-G)^2, sum A, sum A^2) with A = G - V.
 * kind 1 = continuous actor (n_in 13, n_out 1, tanh*out_std + out_mean): reads value[M],
 *          act, logp_old and the GLOBAL (sum A, sum A^2) in stats[0..1];
 *          grad = d(clip surrogate)/dW, sums[0] += sum of surrogate terms.
 * kind 2 = choice actor (n_in <= 64, n_out 2, pairwise softmax): reads value, logp_old,
 *          stats and the GLOBAL action counts counts[0..1] (float64);
 *          grad = d(O(M) Categorical surrogate / M_global^2)/dW, sums[0] += its sum.
 *          counts == NULL selects the opt-in per-row loss: act[M] (0/1 as
 *          float) is read and each row contributes its own action's surrogate / M_global.
 * grad: packed torch layout W1 b1 W2 b2 W3 b3 W4 b4 (32 n_in + 4224 + 33 n_out floats).
 * m_global = the global row count (data parallel: all ranks' rows).
 * Heads with n_in <= 54 run on bf16 MFMA with every f32 operand split exactly into three
 * bf16 parts (products to f32 accuracy; X must then be 16-byte aligned); kind |
 * MHPPO_TRAIN_EXACT_F32 selects the f32-MFMA kernel, whose sums are k-ordered fmaf chains
 * (wider heads always run on it).
 * Per-device, per-stream workspace (up to 4 streams per device): calls on one stream are ordered by
 * it, calls on different streams may run concurrently (MHPPO_EINVAL for a fifth stream). */
#define MHPPO_TRAIN_EXACT_F32 0x100
int mhppo_mlp_train(int kind, int n_in, const float *packed, const float *X, int64_t M, const float *ret,
                    float *value, const float *act, const float *logp_old, const double *stats,
                    const double *counts, double m_global, float out_mean, float out_std, float *grad,
                    double *sums, void *stream);

/* One epoch step of a continuous head run as a pipeline (Algo_PPO.train_model_c :778-815, epochs
 * e and e + 1 overlapped): the ACTOR pass of epoch e (kind 1 of mhppo_mlp_train: advantage
 * A = ret - value normalised with `stats`, the critic pass e's (sum A, sum A^2) over m_global
 * rows) and the CRITIC pass of epoch e + 1 (kind 0, with the critic's weights after its Adam step
 * e) in ONE launch over the same rows: one input load per tile for both nets.  `value` holds V_e
 * on entry and V_{e+1} on return (each row is read before it is overwritten).  grad_* / sums_*
 * as mhppo_mlp_train's (sums_actor += (sum surrogate, 0, 0), sums_critic += (sum (V-G)^2,
 * sum A, sum A^2) of epoch e + 1).  bf16x3 split-precision kernel only (13 inputs, 1 output). */
int mhppo_mlp_train_pair(const float *packed_actor, const float *packed_critic, const float *X, int64_t M,
                         const float *ret, float *value, const float *act, const float *logp_old,
                         const double *stats, double m_global, float out_mean, float out_std,
                         float *grad_actor, double *sums_actor, float *grad_critic, double *sums_critic,
                         void *stream);

/* Critic MSE (:808-809): loss += sum (V-G)^2, dV = 2 (V-G) * inv_m. */
int mhppo_mse_fwd_bwd(const float *value, const float *ret, int64_t M, double inv_m, float *dv,
                      double *loss, void *stream);

/* ---- batched head forward and PPO diagnostics (csrc/mlp_infer.hip; opt-in, beyond the reference) ---- */

/* Forward of one Model_PPO head over M rows in the rollout's arithmetic (bit-identical to what
 * mhppo_rollout_begin / _policy compute for the same feature row and weights): every output is
 * the ascending-k float32 fmaf chain from 0 with the bias added last, on f32 MFMA in 32-row tiles,
 * then the head's finish (kind 1: tanh * std + mean; kind 2: pairwise softmax).  Replaces
 * Model_PPO.forward (Coop-MH-PPO-scalable.py:69-93) on a batch, without autograd.
 * X float32 [M, n_in], n_in <= 64 (any 4-byte alignment); out float32 [M] (kind 0: V, kind 1: mu)
 * or [M, 2] (kind 2: probs).  M == 0 launches nothing.  MHPPO_EINVAL: n_in outside 1..64, a
 * kind / n_out mismatch (kinds 0 and 1: n_out 1, kind 2: n_out 2), a NULL pointer. */
int mhppo_mlp_forward(const mhppo_mlp *net, const float *X, int64_t M, float *out, void *stream);

/* PPO diagnostics of one head over M rows of its batch: the actor's and the critic's forward (one
 * load of X per tile, both nets' weights resident in LDS) and float64 sums of the per-row terms
 * below; no per-row output.  With logp_new the actor's log-probability of the taken action
 * (kind 1: MVN(mu, 0.5).log_prob(act); kind 2: log clamp(p_a / (p0 + p1), eps, 1 - eps), both as
 * the rollout computes them) and V the critic's output.  The reference has no counterpart (it
 * prints reward averages only, :894-906); the quantities are the usual PPO monitors of
 * train_model_c / _d's ratio (:795-806, :834-842) and critics. */
#define MHPPO_DIAG_DSUM   0  /* sum d                           d = logp_new - logp_old          */
#define MHPPO_DIAG_K3     1  /* sum (expm1(d) - d)              >= 0, the low-variance KL estimate */
#define MHPPO_DIAG_CLIP   2  /* rows with ratio outside [0.8, 1.2], as a double                    */
#define MHPPO_DIAG_RATIO  3  /* sum exp(d)                                                         */
#define MHPPO_DIAG_ENT    4  /* kind 2: sum of the policy entropy; kind 1: 0                       */
#define MHPPO_DIAG_E      5  /* sum (G - V)                                                        */
#define MHPPO_DIAG_E2     6  /* sum (G - V)^2                                                      */
#define MHPPO_DIAG_G      7  /* sum G                                                              */
#define MHPPO_DIAG_G2     8  /* sum G^2                                                            */
#define MHPPO_DIAG_V      9  /* sum V                                                              */
#define MHPPO_DIAG_N     10
/* Bytes of device scratch (8-byte aligned) mhppo_ppo_diag needs for M rows (>= 8). */
int64_t mhppo_ppo_diag_work_bytes(int64_t M);
/* actor->kind 1: act float32 [M]; actor->kind 2: act int32 [M]; critic->kind 0, same n_in as the actor.
 * sums float64 [MHPPO_DIAG_N] is WRITTEN (this rank's rows; the sums add across ranks): per-block
 * float64 partials folded in a fixed order (no atomics: the same call gives the same bits).
 * M == 0 writes zeros and launches nothing else.  MHPPO_EINVAL as mhppo_mlp_forward, and for
 * actor and critic of different n_in or an actor of kind 0 / a critic of another kind. */
int mhppo_ppo_diag(const mhppo_mlp *actor, const mhppo_mlp *critic, const float *X, int64_t M,
                   const void *act, const float *logp_old, const float *ret, double *sums,
                   void *work, void *stream);

/* The KL measurement of the opt-in early stop (Algo_PPO(target_kl=...)): the actor half of
 * mhppo_ppo_diag alone, for a launch per head and epoch.
 * Contract: sums float64 [2] is WRITTEN, not accumulated (this rank's rows; the sums add across ranks):
 *   sums[0] = sum d,  sums[1] = sum (expm1(d) - d),  d = logp_new - logp_old,
 * bit for bit mhppo_ppo_diag's sums[MHPPO_DIAG_DSUM] and sums[MHPPO_DIAG_K3] for the same actor, rows
 * and M, whatever critic that call gets: the same grid (a function of M alone), tile-to-wave walk,
 * per-row terms, per-wave tree, wave order and fold.  One weight image and one forward per tile, two
 * float64 accumulators; neither a critic nor `ret` is read.
 * actor->kind 1: act float32 [M]; actor->kind 2: act int32 [M].  work: mhppo_ppo_kl_work_bytes(M)
 * bytes of device scratch (8-byte aligned, >= 8).  M == 0 writes two zeros and launches nothing else.
 * MHPPO_EINVAL as mhppo_ppo_diag: an actor of kind 0, n_in outside 1..64, a kind / n_out mismatch, a
 * NULL pointer, M < 0; a refused call touches nothing. */
int64_t mhppo_ppo_kl_work_bytes(int64_t M);
int mhppo_ppo_kl(const mhppo_mlp *actor, const float *X, int64_t M, const void *act,
                 const float *logp_old, double *sums, void *work, void *stream);

/* ---- GAE(lambda) targets (csrc/mlp_gae.hip; opt-in, beyond the reference, which trains on the
 * Monte-Carlo reward-to-go of mhppo_returns_scan_tm, futur_rewards :658-684) ---- */

/* lambda-return targets over time-major records.  obs_tm float32 [T, B, n_in], rew_tm float64 [T, B],
 * pos int64 [B] / bucket int8 [B] as mhppo_bucket_plan writes them (record b is used iff pos[b] >= 0;
 * its critic is critic[bucket[b]]); pos == NULL: every record is used, with critic0 (critic1 and
 * bucket may then be NULL).  ret_tm float32 [T, B] is written for every record (0 where pos[b] < 0);
 * value_tm float32 [T, B] or NULL receives the critic outputs the scan used (0 where unused).
 * V_t of a record is bit for bit what mhppo_mlp_forward returns for that row and critic (kind 0);
 * the recurrence per record runs in float64, in this operation order (no contraction):
 *   nv = 0; A = 0; c = gamma * lambda
 *   for t = T-1 .. 0:  v = (double)V_t;  d = (rew[t] + gamma * nv) - v;  A = d + c * A;
 *                      ret[t] = (float)(A + v);  nv = v
 * i.e. ret = GAE advantage + V_old, without a bootstrap past step T-1 (the episode's time limit is
 * terminal, as in the reward-to-go; lambda = 1 gives the reward-to-go up to float64 rounding).
 * The train kernels form A = ret - V themselves, so these targets need no other change.
 * A wave walks t backwards for 32 consecutive records (up to 1024 such tiles: one wave per tile and
 * critic, the same operations per record); no atomics, nothing depends on the grid:
 * the same call gives the same bits on any stream, and so does the batch split at a multiple of
 * 32 records.  Observation rows of unused records are read but cannot influence another record.
 * B == 0 launches nothing.  MHPPO_EINVAL: a NULL required pointer, T < 1, B < 0, a critic of kind
 * != 0, n_in outside 1..64, two critics of different n_in, bucket == NULL with pos != NULL, gamma
 * or lambda outside [0, 1] or NaN. */
int mhppo_gae_tm(const mhppo_mlp *critic0, const mhppo_mlp *critic1, const float *obs_tm,
                 const double *rew_tm, const int64_t *pos, const int8_t *bucket, int64_t B, int32_t T,
                 double gamma, double lambda, float *ret_tm, float *value_tm, void *stream);

/* ---- streaming evaluation statistics (csrc/eval_stats.hip; opt-in, beyond the reference, whose
 * get_average (Coop-MH-PPO-scalable.py:1550-1675) reads whole trajectories back) ---- */

/* What get_average's dict needs, reduced on the device to MHPPO_EVS_N float64 sums without keeping
 * a trajectory: counts (integer-valued float64, exact below 2^53) and the first and second moments
 * of the terms get_average hands to its reductions, each term computed as get_average computes it
 * (float32 comparisons and differences; 0.3-step sums in float64; csrc/eval_stats_terms.h) and
 * widened to float64 before it is added.  The moments are plain sums, about no pivot: the terms
 * are speeds, accelerations and times of a few tens at most, so the variance's cancellation
 * S2 - S^2 / n costs ~n 2^-53 relative to the mean square, far below float32.  The sums add across
 * ranks.  mhppo.stats.stats_from_sums turns them into the dict.
 * Episodes are the true ones (one per env from row 0 to row T - 1), not get_average's maximal runs of
 * equal crosswalk width; the two agree whenever consecutive episodes differ in width. */
#define MHPPO_EVS_ROWS       0  /* rows                                                   */
#define MHPPO_EVS_V0         1  /* sum over rows of car 0's speed                         */
#define MHPPO_EVS_V0_SQ      2  /*   ... squared                                          */
#define MHPPO_EVS_ABSA0      3  /* sum over rows of |car 0's acceleration|                */
#define MHPPO_EVS_A0         4  /* sum over rows of car 0's acceleration                  */
#define MHPPO_EVS_A0_SQ      5  /*   ... squared                                          */
#define MHPPO_EVS_ABSVP0     6  /* sum over rows of |pedestrian 0's speed|                */
#define MHPPO_EVS_ABSVP0_SQ  7  /*   ... squared                                          */
#define MHPPO_EVS_EPISODES   8  /* episodes closed                                        */
#define MHPPO_EVS_N_PED      9  /* (episode, pedestrian) entries                          */
#define MHPPO_EVS_PEDT      10  /* sum of the pedestrians' pass times (float32)           */
#define MHPPO_EVS_PEDT_SQ   11
#define MHPPO_EVS_WAIT      12  /* sum of the waiting times (float64), n = N_PED          */
#define MHPPO_EVS_WAIT_SQ   13
#define MHPPO_EVS_N_CAR     14  /* (episode, car) entries                                 */
#define MHPPO_EVS_CART      15  /* sum of the cars' pass times (float32)                  */
#define MHPPO_EVS_CART_SQ   16
#define MHPPO_EVS_FC        17  /* sum of fci - fcn over peds and cars, n = N_PED + N_CAR */
#define MHPPO_EVS_IC        18  /* sum of max fci - max fcn per episode, n = EPISODES     */
#define MHPPO_EVS_N_YSPEED  19  /* pairs of episodes whose car yields (light 1 at row 1)  */
#define MHPPO_EVS_YSPEED    20  /* sum of that car's speed at the pair's first row        */
#define MHPPO_EVS_YSPEED_SQ 21
#define MHPPO_EVS_N_YTIME   22  /* those pairs at which the car passes the crosswalk      */
#define MHPPO_EVS_YTIME     23  /* sum of their times k * 0.3 (float32)                   */
#define MHPPO_EVS_YTIME_SQ  24
#define MHPPO_EVS_YIELD     25  /* car decisions (light at row T - 2) equal to 1          */
#define MHPPO_EVS_GO        26  /*   ... equal to -1                                      */
#define MHPPO_EVS_N_CS      27  /* could_stop entries (light at row 1 < 0)                */
#define MHPPO_EVS_CS        28  /*   ... that could stop                                  */
#define MHPPO_EVS_SC_YY     29  /* two cars: both yield                                   */
#define MHPPO_EVS_SC_GG     30  /*   both go                                              */
#define MHPPO_EVS_SC_GY     31  /*   car 0 goes, car 1 yields                             */
#define MHPPO_EVS_SC_YG     32  /*   car 0 yields, car 1 goes                             */
#define MHPPO_EVS_N         33

/* Bytes of the caller-owned device state (8-byte aligned) for this env's N, S, P:
 * N * (8 MHPPO_EVS_N + 4 (1 + 2 P + 5 nb_car) + 4 (2 P + nb_car)), i.e. per env the float64
 * accumulators, the previous row's fields the pair tests need and the episode's counters.
 * MHPPO_EINVAL (negative) for the 4cars / 4cars2 layouts, which get_average is not defined for. */
int64_t mhppo_eval_stats_bytes(const mhppo_env *env);
/* Zero the state (accumulators and carry). */
int mhppo_eval_stats_begin(mhppo_env *env, void *state, void *stream);
/* Consume row t (0 <= t < T) of the current episode of every env: obs float32 [N, obs_dim], the
 * pre-step observation mhppo_eval_step copies into obs_hist[t] (bufs->obs before the step), or a
 * row of a recorded trajectory.  t == 0 opens an episode, t >= 1 closes the pair (t - 1, t),
 * t == T - 1 closes the episode into the env's accumulators.  Rows of one episode must arrive in
 * order.  One lane per env; a block stages its envs' rows through LDS in one coalesced copy.
 * MHPPO_EINVAL: T < 2, t outside [0, T), a NULL pointer, an unsupported layout. */
int mhppo_eval_stats_row(mhppo_env *env, const float *obs, int t, int T, void *state, void *stream);
/* sums float64 [MHPPO_EVS_N] (device) is WRITTEN with the per-env accumulators folded over the envs
 * in a fixed order (one block per sum, a fixed env-to-thread assignment and a fixed tree: no atomics,
 * the same call gives the same bits on any stream).  The state is left as it is: more rows may follow. */
int mhppo_eval_stats_fold(mhppo_env *env, const void *state, double *sums, void *stream);

/* ---- gradient-norm clipping and the Adam step (csrc/adam_clip.hip; opt-in, beyond the reference,
 * which steps torch.optim.Adam on unclipped gradients, Coop-MH-PPO-scalable.py:806-815) ---- */

/* One launch measures the gradient norm of each of n_nets independent nets, clips it to max_norm
 * and applies one Adam step to the net, on the torch optimisers' own state tensors: it replaces
 * torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm) + optimizer.step() per net.
 * A net is an ordered list of up to MHPPO_ADAM_MAX_SEGS segments (Model_PPO: the eight tensors
 * W1 b1 .. W4 b4 in flat order); a segment's param / grad / exp_avg / exp_avg_sq are separate float32
 * allocations of n elements, `step` is torch's float32 scalar.  The net's flat element index i runs
 * 0 .. n_total - 1 across the segments in order (n_total <= 2^30).
 * The table is HOST memory (the one exception to the convention above): it travels in the kernel
 * arguments (8 nets x 8 segments x 48 bytes, under the 4 KB a launch takes), so there is no device
 * table to upload, keep alive or invalidate when an optimiser's state is replaced.
 *
 * Arithmetic contract, per net, independent of the other nets of the call (mhppo.ppo.adam_clip_torch
 * restates it in torch and is compared with the kernel bit for bit):
 *   ss    = the fold of (double)g_i * (double)g_i (exact) over i = 0 .. n_total - 1 in the order of
 *           k_fold<1024, 4> (csrc/block_prims.h): thread b's chain u adds elements b + 1024 u,
 *           b + 1024 u + 4096, ... from +0.0; (a0 + a1) + (a2 + a3); the 1024-thread halving tree
 *   norm  = sqrt(ss) in float64;  norms[k] = norm  (the norm BEFORE clipping)
 *   coef  = max_norm / (norm + 1e-6);  s = coef < 1.0 ? (float)coef : 1.0f
 *           (max_norm = +inf clips nothing and only reports the norms; a NaN coef leaves s = 1)
 *   per element, float32, no contraction, division and square root correctly rounded:
 *     g' = g * s
 *     m  = m + (g' - m) * c1                 c1 = (float)(1 - beta1)
 *     v  = v * b2 + (g' * g') * c2           b2 = (float)beta2, c2 = (float)(1 - beta2)
 *     den = sqrtf(v) / q + e                 q  = (float)bias2, e = (float)eps
 *     p  = p - a * (m / den)                 a  = (float)alpha
 *   every segment's step = (float)t.  grad is read and never written.
 * alpha = lr / (1 - beta1^t) and bias2 = sqrt(1 - beta2^t) come from the caller, in float64, for
 * the step count t AFTER the increment (a device pow would not be reproducible on the host).
 * This is torch.optim.Adam with weight_decay 0, no amsgrad, no maximize, up to the rounding of
 * the two bias corrections (torch._fused_adam_ forms them on the device).  There is no skip logic:
 * a non-finite gradient makes norm inf or NaN, hence s = 0 or 1, and poisons its own net's
 * moments and parameters through g' as the arithmetic above says (a NaN's sign and payload are
 * the hardware's); other nets are unaffected.
 * One block of 1024 threads per net folds, then steps the same net: no block waits on another, no
 * atomics, nothing depends on the grid: the same call gives the same bits on any stream, whichever
 * other nets share it.  n_nets == 0 launches nothing.
 * MHPPO_EINVAL: nets or norms NULL, n_nets outside 0 .. MHPPO_ADAM_MAX_NETS, n_seg outside
 * 0 .. MHPPO_ADAM_MAX_SEGS, a segment with n < 0 or (n > 0) a NULL pointer, n_total > 2^30,
 * max_norm NaN or <= 0, a beta outside [0, 1) or NaN. */
#define MHPPO_ADAM_MAX_NETS 8  /* the product steps at most 6 (three heads' actors and critics) */
#define MHPPO_ADAM_MAX_SEGS 8
typedef struct mhppo_adam_seg {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    float *step;
    int64_t n;
} mhppo_adam_seg;
typedef struct mhppo_adam_net {
    mhppo_adam_seg seg[MHPPO_ADAM_MAX_SEGS];
    int32_t n_seg, reserved;
    int64_t t;                 /* the step count after this step's increment */
    double alpha, bias2;       /* lr / (1 - beta1^t), sqrt(1 - beta2^t) */
    double beta1, beta2, eps;
} mhppo_adam_net;
int mhppo_adam_clip(const mhppo_adam_net *nets, int32_t n_nets, double max_norm, double *norms, void *stream);

/* mhppo_adam_clip with a per-net gate decided on the device (the KL early stop of
 * Algo_PPO(target_kl=...): the host never reads the KL, so an update's epoch loop has no round trip).
 * Contract: gates == NULL, or a net whose gate has kl == NULL: the net follows mhppo_adam_clip's
 * contract bit for bit.  A gated net is OPEN iff *stop == 0 and kl[1] <= limit (a NaN kl closes):
 *   open:    mhppo_adam_clip's contract bit for bit; *stop stays 0.
 *   closed:  norms[k] = NaN (a net that was not stepped); *stop = epoch if it was 0 (so a stop is
 *            sticky and keeps the first epoch); nothing else of the net is read or written: param,
 *            exp_avg, exp_avg_sq and step keep their bits, grad is not read, the fold is skipped.
 * The decision is the same in every thread of the net's block: all threads read *stop, a barrier,
 * then one thread writes it.  kl and stop are DEVICE memory, read when the kernel runs (stream
 * order: after the mhppo_ppo_kl launch and any all-reduce that fill kl); the gates array is HOST
 * memory and travels with the table in the kernel arguments (8 x 32 bytes more: 3 664 bytes of the
 * 4 KB in all).  limit is in the units of kl[1], a SUM over rows (mhppo.ppo.kl_limit: 1.5 tau m):
 * the kernel never divides.  Nets stay independent and the call deterministic, as mhppo_adam_clip's.
 * MHPPO_EINVAL: everything mhppo_adam_clip refuses, and a gated net with stop == NULL, epoch < 1 or
 * limit NaN or < 0 (inf allowed: it never closes on a finite kl); a refused call touches nothing. */
typedef struct mhppo_adam_gate {
    const double *kl;  /* device: the 2 doubles of mhppo_ppo_kl (global sums); NULL: this net is not gated */
    double limit;      /* open iff *stop == 0 and kl[1] <= limit (a NaN kl closes) */
    int32_t *stop;     /* device word, 0 = running */
    int32_t epoch;     /* >= 1: written to *stop by the call that first closes the net */
    int32_t reserved;
} mhppo_adam_gate;
int mhppo_adam_clip_gated(const mhppo_adam_net *nets, int32_t n_nets, double max_norm, double *norms,
                          const mhppo_adam_gate *gates, void *stream);

/* ---- the minibatch shuffle (csrc/batch_shuffle.hip, csrc/batch_shuffle.h; opt-in, beyond the
 * reference, whose epochs are full-batch) ---- */

/* Destination row i is source row perm(key, M, i), for X [M, n_in] float32 (n_in 1 .. 64) and the
 * three 4-byte columns act, logp, ret [M]; perm is a stateless keyed bijection of [0, M): nothing
 * is drawn, sorted or kept between calls, the same (key, M) gives the same rows on any stream.
 *   h = max(1, ceil(bitlen(M - 1) / 2)), mask = 2^h - 1   (the walk domain 4^h is >= M, < 4 M for M >= 2)
 *   round keys k_0 .. k_7: the four Philox-4x32-10 words of counter 0 under `key` (the noise's
 *     block and key layout, mhppo_philox_uniform), then those of counter 1
 *   one pass over x: (L, R) = (x >> h, x & mask); for r = 0 .. 7: (L, R) <- (R, L ^ (fmix32(R ^ k_r) & mask));
 *     x = L << h | R;  fmix32 is the murmur3 finaliser (^= >> 16, *= 0x85EBCA6B, ^= >> 13, *= 0xC2B2AE35, ^= >> 16)
 *   perm(key, M, i): the pass applied to i, and again while the result is >= M (cycle-walk)
 * The act column is copied bitwise (float32 of the continuous heads, int32 of the choice head), as
 * are logp, ret and X: NaN payloads and signed zeros survive.
 * K >= 1 is the number of slices the caller will cut the shuffled batch into: slice j holds the
 * rows [b_j, b_{j+1}), b_j = 4 floor(j ceil(M / 4) / K) for j < K, b_K = M: every slice starts at a
 * multiple of 4 rows (16-byte aligned for the train kernels whatever n_in is); slices are empty
 * when M < 4 K.  K matters to `counts` alone.
 * counts: NULL, or float64 [K][2]; act is then int32 and counts[j] = (the rows of slice j with
 * act == 0, with act == 1), folded in csrc/block_prims.h's fixed order by one block per slice in a
 * second launch, no atomics (M <= 2^30 with counts).
 * M == 0 launches nothing; counts, if given, is zeroed.  M <= 2^31 - 1.
 * Sources need 4-byte alignment only (a bucket that starts at any row of a shared buffer);
 * destinations must be 16-byte aligned.
 * MHPPO_EINVAL, nothing written: n_in outside 1 .. 64, K < 1, M out of range, and for M > 0 a NULL
 * source or destination, a source not 4-byte or a destination not 16-byte aligned, a source range
 * that overlaps a destination range. */
int mhppo_batch_shuffle(int32_t n_in, int64_t M, const float *X, const void *act, const float *logp,
                        const float *ret, uint64_t key, int32_t K, float *X_out, void *act_out, float *logp_out,
                        float *ret_out, double *counts, void *stream);

/* ---- stateless policy inference (csrc/policy_infer.hip, csrc/policy_rule.h; opt-in, beyond the
 * reference, whose only way from the heads to an action is Env_rollout.iterations :152-252 on its own
 * env) ---- */

/* The deterministic policy of mhppo_eval_step as a function of observation rows: no env handle, the
 * rows may come from anywhere (another simulator, a recorded trajectory, a grid).  `cfg` names the
 * observation layout and the constants of the rule (variant, nb_car, nb_ped, nb_lines, dt, car_b);
 * n_envs, the seeds and flags are ignored.  It gets mhppo_env_create's variant and shape checks.
 * The calls run on the current device.
 *
 * The rule (csrc/policy_rule.h), per row o with S slots and P pedestrians:
 *   decide  a_d[i][p] = (p1 > p0) of softmax(choice(obs_car_ped_d(o, i, p)))   (the first maximum)
 *   act     for each slot i:  a = car_b[1][0];  for p = 0 .. P - 1:
 *             f = obs_car_ped(o, i, p)                                          (13 features)
 *             cand = f[7] != 0 ? max(car_b[0][0], min(car_b[1][0], (10 - f[0]) / dt))    (float64)
 *                              : (double)(tanh(head(f)) * std + mean), head = wait if 2 a_d[i][p] - 1 > 0
 *                                                                             else cross
 *             if (cand < a) a = cand;  lim = (10 - (double)f[0]) / dt;  if (lim < a) a = lim
 *           actions[i] = a
 *   lights  actions[S + i] = 2 a_d.flat[i] - 1: the FLAT index i into the row's [S, P] block, not
 *           [i][0] (the reference's quirk, :188, :210; the two differ when P > 1)
 * Comparisons with NaN are false: a NaN head output changes nothing and is reported nowhere.
 * Every head output is bit for bit mhppo_mlp_forward's for the same feature row, and actions are
 * bit for bit what mhppo_eval_step hands its env step for the same o and a_d.  When a choice is
 * re-decided is the caller's schedule (mhppo.policy.PolicySession restates mhppo_eval_step's).
 * Both launches walk 32-triple tiles on f32 MFMA; the feature rows are built in LDS from the
 * observation rows and never written to memory.  No atomics, nothing depends on the grid: the
 * same call gives the same bits on any stream.  M == 0 launches nothing and touches nothing.
 * obs needs 4-byte alignment only. */

/* out = (obs_dim, S, P, choice_dim) of a config; no device is touched. */
int mhppo_policy_dims(const mhppo_env_cfg *cfg, int32_t out[4]);
/* obs float32 [M, obs_dim]; a_d int32 [M, S, P]; probs float32 [M, S, P, 2] or NULL.
 * MHPPO_EINVAL: a refused config, actor_choice not kind 2 with n_in == choice_dim (<= 64) and n_out 2,
 * a NULL pointer, M < 0. */
int mhppo_policy_decide(const mhppo_env_cfg *cfg, const mhppo_mlp *actor_choice, const float *obs, int64_t M,
                        int32_t *a_d, float *probs, void *stream);
/* actions float64 [M, 2S] = [acc_0 .. acc_{S-1}, light_0 .. light_{S-1}], the layout mhppo_env_step takes.
 * MHPPO_EINVAL: a refused config, nb_ped > 32 (a slot's pedestrians share one tile), an actor not
 * kind 1 with 13 inputs and 1 output, a NULL pointer, M < 0. */
int mhppo_policy_act(const mhppo_env_cfg *cfg, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                     const float *obs, const int32_t *a_d, int64_t M, double *actions, void *stream);

/* ---- stochastic policy sampling (csrc/policy_infer.hip, csrc/policy_sample_rule.h; opt-in) ---- */

/* The training policy of the collector (mhppo_rollout_begin / _policy / _sample_env) as a function of
 * observation rows: no env handle, nothing written but the outputs named here.  `cfg`, the device and
 * obs's alignment are mhppo_policy_decide's.
 *
 * The rule (csrc/policy_sample_rule.h), per row o:
 *   decide  (slot i, ped p): (p0, p1) = softmax(choice(obs_car_ped_d(o, i, p))); n = p / (p0 + p1);
 *             a_d = u >= n[0] (or the forced value); logp_d = logf(clamp(n[a_d], eps, 1 - eps))
 *           (slot i): closest = closest_ped_d(o, i); exist = the car's exist field != 0 (scalable), else 1
 *   act     (slot i): loc = 2.0f, sel = 0; for p = 0 .. P - 1 (scalable: pedestrians whose exist field
 *             is 0 take no part): out = tanh(head(obs_car_ped(o, i, p))) * std + mean, head = wait if
 *             2 a_d[i][p] - 1 > 0 else cross; loc = torch.minimum(loc, out); if (out == loc) sel = p
 *           a = loc + L eps; logp = MVN(loc, 0.5).log_prob(a)                          (float32)
 *           actions[i] = a; actions[S + i] = 2 a_d[i][closest[i]] - 1 (a closest outside [0, P): 0)
 *           feat_c[i] = obs_car_ped(o, i, sel)
 * No left-lane override and no speed cap.  An absent car slot of the scalable variant (exist 0) is
 * computed as any other slot, as the collector does (its action reaches the env step); the collector
 * keeps no record of it, so its act, logp and feat_c are the caller's to mask with `exist`.  status (uint32 [1] or NULL; only ever OR-ed into): bit 1 for NaN
 * choice probabilities, bit 2 for a NaN loc, as mhppo_rollout_check reads them.
 * On present slots every output is bit for bit what the collector records for the same row, weights
 * and noise (logp_d within the device logf's rounding of the host's).
 *
 * mhppo_policy_noise: `tape` (decide: u float32 [M, S, P]; act: eps float32 [M, S]) or, for decide,
 * `forced` (int32 [M, S, P]: the decisions themselves) when set; with both NULL the draw is made in
 * the kernel, Philox-4x32-10 under `key` at the collector's counters (mhppo_philox_uniform /
 * _normal as RolloutGPU.draw_noise calls them): row r is env first_env + r,
 *   u(r, i, p)   counter (first_env + r) S P + i P + p
 *   eps(r, i)    counter (t + 1) 2^40 + (first_env + r) S + i
 * and key = seed * 1000003 + iteration (mod 2^64). */
typedef struct mhppo_policy_noise {
  const float *tape;
  const int32_t *forced;
  uint64_t key, first_env;
  int64_t t; /* act, Philox form: the step (>= 0) */
} mhppo_policy_noise;

/* a_d int32, logp_d float32 [M, S, P]; probs float32 [M, S, P, 2], feat_d float32 [M, S, P, choice_dim]
 * and status may be NULL (their stores are skipped); closest int32, exist uint8 [M, S].
 * MHPPO_EINVAL: as mhppo_policy_decide; a NULL noise, or one with both tape and forced. */
int mhppo_policy_sample_decide(const mhppo_env_cfg *cfg, const mhppo_mlp *actor_choice, const float *obs, int64_t M,
                               const mhppo_policy_noise *noise, int32_t *a_d, float *logp_d, float *probs,
                               float *feat_d, int32_t *closest, uint8_t *exist, uint32_t *status, void *stream);
/* actions float64 [M, 2S]; act, logp float32 [M, S]; feat_c float32 [M, S, 13] and status may be NULL.
 * MHPPO_EINVAL: as mhppo_policy_act; a NULL noise, one with forced set, or the Philox form with t < 0. */
int mhppo_policy_sample_act(const mhppo_env_cfg *cfg, const mhppo_mlp *actor_cross, const mhppo_mlp *actor_wait,
                            const float *obs, const int32_t *a_d, const int32_t *closest, int64_t M,
                            const mhppo_policy_noise *noise, double *actions, float *act, float *logp, float *feat_c,
                            uint32_t *status, void *stream);

/* ---- external rollouts: the record pass (csrc/rollout_record.hip; opt-in, beyond the reference,
 * whose rollout owns its env) ---- */

/* The collector's bookkeeping between a sampling step and the bucketing, for M parallel streams of
 * S slots whose observation rows and rewards come from outside the library: what
 * mhppo_rollout_begin and mhppo_rollout_sample_env keep of an episode, without an env handle.
 * Segment s = row * S + slot, NS = M S <= 2^31 - 1.  The calls run on the current device.
 *
 * begin   ep_min[s] = +0.0 for every s (float64 [M, S]).  With rec_of (int32 [NS + M + 1]; NULL: the
 *         identity layout) the compact record layout of mhppo_rollout_bufs.rec_of, from exist (uint8
 *         [M, S]): rec_of[s] = the number of s' < s with exist[s'] != 0 if exist[s] != 0, else -1;
 *         rec_of[NS + r] = the number of s' < r S with exist[s'] != 0, r = 0 .. M.  Bit for bit what
 *         mhppo_rollout_begin writes for the same exist.
 *         work: mhppo_record_work_bytes(M, S) bytes of device scratch, 8-byte aligned, the caller's
 *         own (needed with rec_of only): calls on different streams with different work buffers are
 *         independent.  Two small launches and a memset; no atomics, nothing depends on the grid.
 * step    step t < T of the episode, one launch.  In: act, logp float32 [M, S] and feat_c float32
 *         [M, S, 13] as mhppo_policy_sample_act writes them, rew and rew_light float64 [M, S] as the
 *         simulator's step returns them.  The time-major records obs_c_tm float32 [T, NS, 13],
 *         act_tm, logp_tm float32 [T, NS], rew_tm float64 [T, NS]: segment s goes to record
 *         t NS + r, r = s with rec_of NULL (every segment is stored), else r = rec_of[s] (nothing is
 *         stored for rec_of[s] < 0).  The copies are bitwise: NaN payloads and signed zeros survive.
 *         For EVERY segment, stored or not, with m = ep_min[s] and x = rew_light[s]:
 *           ep_min[s] = (m != m) ? m : ((x != x) ? x : (x < m ? x : m))
 *         (np.minimum: a NaN stays, and of +0.0 and -0.0 the old value stays).
 *         rec_of must be one that begin (or mhppo_rollout_begin) wrote: the kernel relies on the
 *         ranks of consecutive present segments being consecutive, and stores a block of 256
 *         segments' records as one contiguous run per array (16-byte stores between the run's
 *         ends; the arrays need their natural alignment only).  A block whose run would leave
 *         [0, NS) stores no records.  No atomics, nothing depends on the grid.
 * M == 0 launches nothing and touches nothing.
 * MHPPO_EINVAL, nothing written: M < 0, S < 1, M S > 2^31 - 1; begin: for M > 0 a NULL ep_min, or
 * rec_of without exist or work; step: t outside [0, T), for M > 0 a NULL pointer other than rec_of. */
int64_t mhppo_record_work_bytes(int64_t M, int32_t S);
int mhppo_record_begin(const uint8_t *exist, int64_t M, int32_t S, int32_t *rec_of, double *ep_min, void *work,
                       void *stream);
int mhppo_record_step(int64_t M, int32_t S, int32_t t, int32_t T, const float *act, const float *logp,
                      const float *feat_c, const double *rew, const double *rew_light, const int32_t *rec_of,
                      float *obs_c_tm, float *act_tm, float *logp_tm, double *rew_tm, double *ep_min, void *stream);

/* ---- early episode ends of external rollouts (opt-in: ExternalRollout(early_end=True); the calls
 * above keep their launches and their bits) ----
 * done is per stream: uint8 [M], what a vectorised simulator's step returns.  If stream r first reports
 * done at step t, step t is its last and its length is L_r = t + 1; done is terminal exactly as the time
 * limit is (V = 0 after it; a truncation that bootstraps: the section after this one); a done raised again
 * later is ignored.  len int32 [M]: 0 =
 * still running (the caller memsets it to 0 when an episode begins), else L_r.  After k recorded steps
 * the effective length of stream r is len[r] ? len[r] : k.  All row offsets are int64. */

/* mhppo_record_step with done: the step's records are stored exactly as mhppo_record_step stores them,
 * for EVERY segment, finished or not (a block's records stay one contiguous run; the ragged calls
 * below never read a record at or past its stream's length).  ep_min[s] is updated only for segments
 * whose stream was running on entry; len[r] = t + 1 for streams that were running on entry and have
 * done[r] != 0.  Running on entry to step t: len[r] == 0 or len[r] == t + 1 -- steps are recorded once
 * each, in order from 0, so t + 1 can only be this very call's write (a stream's segments can sit in
 * two blocks).  One launch, no atomics.  MHPPO_EINVAL: as mhppo_record_step, or done / len NULL for
 * M > 0. */
int mhppo_record_step_done(int64_t M, int32_t S, int32_t t, int32_t T, const float *act, const float *logp,
                           const float *feat_c, const double *rew, const double *rew_light, const int32_t *rec_of,
                           float *obs_c_tm, float *act_tm, float *logp_tm, double *rew_tm, double *ep_min,
                           const uint8_t *done, int32_t *len, void *stream);

/* The ragged plan: the buckets' rows when every stream has its own length.  In: pos int64 [NS] / bucket
 * int8 [NS] per record column b < NS = M S as mhppo_bucket_plan writes them, rec_of int32 [NS] or NULL
 * (the layout the records were stored in), len int32 [M], k >= 1 the number of recorded steps (a len
 * outside [1, k] counts as k).
 * Out: len_rec int32 [NS] = the effective length of the stream that column b's record belongs to (the
 * stream b / S in the identity layout, the stream of the segment s with rec_of[s] == b in the compact
 * one), 0 for a column that holds no record.  row0 int64 [NS] = the first row of column b's segment in
 * the shared buffer: for a used column (pos[b] >= 0) of bucket 0 the sum of len_rec[b'] over the used
 * bucket-0 columns b' < b; of bucket 1, W0 plus the same sum over bucket-1 columns, W0 = (rows_cross +
 * 3) / 4 * 4 (the wait bucket's 52-byte observation rows start 16-byte aligned); -1 where pos[b] < 0.
 * A segment's rows are contiguous, row0 .. row0 + len_rec - 1; rows_cross + 3 + rows_wait <= NS k + 3.
 * info int64 [2] (device) = {rows_cross, rows_wait}.
 * The rows follow column order; that is the order of pos because mhppo_bucket_plan ranks a bucket's
 * columns in column order, and (compact layout) because rec_of ascends with the segment index.
 * Three launches (per-block sums, a one-block scan, placement): no block waits on another, no
 * atomics.  work: mhppo_ragged_work_bytes(NS) bytes of device scratch, 8-byte aligned.
 * MHPPO_EINVAL: M < 0, S < 1, M S > 2^31 - 1, k < 1, info or work NULL, for M > 0 a NULL pointer other
 * than rec_of. */
int64_t mhppo_ragged_work_bytes(int64_t NS);
int mhppo_ragged_plan(const int64_t *pos, const int8_t *bucket, const int32_t *rec_of, const int32_t *len, int64_t M,
                      int32_t S, int32_t k, int64_t *row0, int32_t *len_rec, int64_t *info, void *work, void *stream);

/* mhppo_returns_scan_tm with a length per column: column b scans t = len_rec[b] - 1 .. 0 from G = 0 and
 * ret[t][b] = 0 for t >= len_rec[b] (len_rec clamped to [0, T]).  len_rec == NULL: mhppo_returns_scan_tm's
 * bits. */
int mhppo_returns_scan_tm_len(const double *rew, float *ret, int64_t B, int32_t T, double gamma,
                              const int32_t *len_rec, void *stream);

/* mhppo_gae_tm with a length per record: record b is used at step t iff pos[b] >= 0 (or pos == NULL) and
 * t < len_rec[b] (clamped to [0, T]); its recurrence starts from A = nv = 0 at t = len_rec[b] - 1; ret and
 * value are 0 at and beyond the length.  V_t stays bit for bit mhppo_mlp_forward's.  len_rec == NULL:
 * mhppo_gae_tm's bits.  Errors as mhppo_gae_tm. */
int mhppo_gae_tm_len(const mhppo_mlp *critic0, const mhppo_mlp *critic1, const float *obs_tm, const double *rew_tm,
                     const int64_t *pos, const int8_t *bucket, int64_t B, int32_t T, double gamma, double lambda,
                     float *ret_tm, float *value_tm, const int32_t *len_rec, void *stream);

/* mhppo_bucket_scatter_sums over ragged segments: record (t, b) with row0[b] >= 0 and t < len_rec[b]
 * (t < T) goes to row row0[b] + t of dst[bucket[b]]; nothing else is written.  rew_sums[bucket[b]] adds
 * (double)(float)rew over exactly those records, per-block partials folded in the fixed order of
 * mhppo_bucket_scatter_sums.  row0 / len_rec as mhppo_ragged_plan writes them; the caller's buffers
 * hold every row row0[b] + len_rec[b] - 1.  work: mhppo_bucket_work_bytes(NS, T) bytes.
 * MHPPO_EINVAL: NS < 0, T <= 0, dst NULL, for NS > 0 any NULL pointer. */
int mhppo_bucket_scatter_ragged(const int64_t *row0, const int8_t *bucket, const int32_t *len_rec, int64_t NS,
                                int32_t T, const float *obs_tm, const float *act_tm, const float *logp_tm,
                                const float *ret_tm, const double *rew_tm, const mhppo_bucket_dst *dst,
                                double *rew_sums, void *work, void *stream);

/* ---- truncation bootstrap of external rollouts (opt-in: ExternalRollout(early_end=True, bootstrap=True);
 * the calls above keep their launches and their bits) ----
 * An episode that is cut -- by a simulator's time limit, by a window's end, by taking the batch while the
 * stream still runs -- has not ended: the value of the state after its last step belongs in its targets.
 * trunc uint8 [M] (the caller memsets it to 0 when an episode begins) says of a stream that reported done
 * whether that done was a truncation: it is set from the simulator's `truncated` flag at the step that
 * first reports done and at no other (if a simulator raises terminated and truncated together, what it
 * passes as truncated decides).  A stream still running after k recorded steps (k = T included) is cut
 * at k; that cut is a truncation iff cut_truncates != 0.  A terminal end keeps V = 0 after it.
 * The successor row s_L of a truncated segment of effective length L: for L < k record L of its column,
 * which mhppo_record_step_done stored (the caller's contract: the row it recorded at step L for a
 * truncated stream is the stream's true successor, not a reset row); for L == k the segment's row of
 * feat_tail float32 [M, S, n_in], the features of the observation after the last recorded step.  The
 * value is the critic's of the segment's bucket, read when the batch is built: before the iteration's
 * update, as the GAE values are.  The choice head's episodic-minimum target and the reward sums do not
 * change. */

/* v_boot of every record column.  Per segment s = r S + i (r < M, i < S):
 *   col   = rec_of ? rec_of[s] : s; for col < 0 nothing is written
 *   ended = 1 <= len[r] <= k;  L = ended ? len[r] : k;  tr = ended ? trunc[r] != 0 : cut_truncates != 0
 *   row   = L < k ? obs_tm[L][col] : feat_tail[s]             (obs_tm float32 [>= k, M S, n_in])
 *   v_boot[col] = (pos[col] >= 0 && tr && (L < k || feat_tail)) ? critic[bucket[col] != 0](row) : 0.0f
 * critic[0] = critic0, critic[1] = critic1; the value is bit for bit mhppo_mlp_forward's for that row and
 * critic.  A row the rule does not select is not read and cannot reach a result (it may hold NaN).
 * Columns that hold no record are not touched: hand in a zeroed v_boot float32 [M S].  feat_tail NULL:
 * segments of effective length k are not bootstrapped.  One launch: four-wave blocks, a 32-segment tile
 * per wave, a grid that is a function of M S alone; no atomics.  M == 0 launches nothing.
 * MHPPO_EINVAL, nothing written: a critic that is NULL, not kind 0 with one output, or of another n_in
 * than the other; M < 0, S < 1, M S > 2^31 - 1; k < 1; for M > 0 a NULL pointer other than rec_of and
 * feat_tail. */
int mhppo_boot_values(const mhppo_mlp *critic0, const mhppo_mlp *critic1, const int64_t *pos, const int8_t *bucket,
                      const int32_t *rec_of, const int32_t *len, const uint8_t *trunc, int64_t M, int32_t S,
                      int32_t k, int32_t cut_truncates, const float *obs_tm, const float *feat_tail, float *v_boot,
                      void *stream);

/* mhppo_returns_scan_tm_len started from a bootstrap value: column b scans t = L - 1 .. 0 from
 * G = (double)v_boot[b] instead of 0, L = len_rec[b] clamped to [0, T]: ret[L - 1][b] = (float)(rew[L - 1][b]
 * + gamma (double)v_boot[b]).  For L == 0 v_boot[b] is not read and the column is all zeros.
 * v_boot == NULL: mhppo_returns_scan_tm_len's launch and bits. */
int mhppo_returns_scan_tm_boot(const double *rew, float *ret, int64_t B, int32_t T, double gamma,
                               const int32_t *len_rec, const float *v_boot, void *stream);

/* mhppo_gae_tm_len started from a bootstrap value: record b's recurrence starts at t = len_rec[b] - 1
 * from nv = (double)v_boot[b] (the value after its last step) and A = 0, so delta there is
 * r + gamma v_boot[b] - V.  len_rec is required with v_boot (MHPPO_EINVAL otherwise).  v_boot == NULL:
 * mhppo_gae_tm_len's launch and bits.  Errors as mhppo_gae_tm. */
int mhppo_gae_tm_boot(const mhppo_mlp *critic0, const mhppo_mlp *critic1, const float *obs_tm, const double *rew_tm,
                      const int64_t *pos, const int8_t *bucket, int64_t B, int32_t T, double gamma, double lambda,
                      float *ret_tm, float *value_tm, const int32_t *len_rec, const float *v_boot, void *stream);

/* ---- auto-reset of external rollouts (opt-in: ExternalRollout(auto_reset=E); the calls above keep
 * their launches and their bits) ----
 * A vectorised simulator resets a stream the moment it reports done: stream r plays episode after episode
 * inside the T-step window.  Stream r owns E >= 1 LANES; lane e of stream r is the e-th episode the stream
 * starts in the window, lane v = e M + r, lane-segment (v, i) = v S + i, E M S <= 2^31 - 1.  Lane 0 starts
 * at step 0.  If stream r reports done at recorded step t while its current lane e runs, the lane ends
 * with len = t + 1 - t0 (terminal: V = 0 after it).  If e + 1 < E and step t + 1 is acted on, lane e + 1
 * starts at t0 = t + 1 with a choice decision of its own, drawn from the row handed to that step (same-step
 * auto-reset: after a done the simulator's row is already the new episode's first).  With e + 1 == E the
 * stream idles for the rest of the window: its records are stored, nothing of them reaches a lane.  The
 * records keep the identity layout at wall-clock time: column r S + i of step t.
 *
 * mhppo_decision: one set of mhppo_policy_sample_decide outputs, for M rows or (lane-major) E M lanes:
 * a_d int32 [., S, P], logp_d float32 [., S, P], probs float32 [., S, P, 2], feat_d float32 [., S, P, dc],
 * closest int32 [., S], exist uint8 [., S].
 * mhppo_lanes: the lanes' arrays.  d (lane-major decisions; exist 0 for a lane never started), ep_min
 * float64 [E M, S], t0 int32 [E M] (0 for a lane never started), len int32 [E M] (0: open, or never
 * started) are what the batch reads; cur int32 [2 M] is private: cur[(t & 1) M + r] is stream r's current
 * lane at step t.  restart(t) reads half (t - 1) & 1 and writes half t & 1, so no thread of a launch reads
 * what another writes.
 *
 * begin    lane 0 of every array of d <- first, every other lane 0; ep_min +0.0; t0, len, cur 0.
 * restart  step t in [1, T), before record(t), once per step and for every step (a caller with E == 1 may
 *          skip them all: nothing can restart).  Stream r restarts iff its current lane e is closed
 *          (len != 0) and e + 1 < E.  For those: every array of lane e + 1 of d and of `current` (the M-row
 *          decision mhppo_policy_sample_act reads) <- fresh's rows of stream r; t0 = t; cur = e + 1.  A
 *          stream that does not restart keeps `current` and its lanes bit for bit.
 * record   step t in [0, T): the step's records exactly as mhppo_record_step stores them in the identity
 *          layout (one contiguous run per block of 256 segments), for every stream, idle or not; the current
 *          lane's ep_min takes mhppo_record_step's minimum if the lane runs on entry; a running lane with
 *          done[r] != 0 closes with len = t + 1 - t0.
 * close    after k >= 1 recorded steps, into arrays of the caller's (lanes is not changed: recording may go
 *          on): len_out[v] = k - t0[v] and cut_out[v] = 1 for a started lane still open, else len[v] and 0.
 * Each is ONE launch; no atomics, nothing depends on the grid, no host read.  M == 0 launches nothing.
 * MHPPO_EINVAL, nothing written: E < 1, M < 0, S < 1, E M S > 2^31 - 1; P < 1 or dc < 1 (begin, restart); t
 * outside its range; k outside [1, T]; for M > 0 any NULL pointer. */
typedef struct {
  int32_t *a_d;
  float *logp_d, *probs, *feat_d;
  int32_t *closest;
  uint8_t *exist;
} mhppo_decision;
typedef struct {
  mhppo_decision d;
  double *ep_min;
  int32_t *t0, *len, *cur;
} mhppo_lanes;
int mhppo_lanes_begin(const mhppo_lanes *lanes, int32_t E, int64_t M, int32_t S, int32_t P, int32_t dc,
                      const mhppo_decision *first, void *stream);
int mhppo_lanes_restart(const mhppo_lanes *lanes, int32_t E, int64_t M, int32_t S, int32_t P, int32_t dc, int32_t t,
                        int32_t T, const mhppo_decision *fresh, const mhppo_decision *current, void *stream);
int mhppo_lanes_record(const mhppo_lanes *lanes, int32_t E, int64_t M, int32_t S, int32_t t, int32_t T,
                       const float *act, const float *logp, const float *feat_c, const double *rew,
                       const double *rew_light, float *obs_c_tm, float *act_tm, float *logp_tm, double *rew_tm,
                       const uint8_t *done, void *stream);
int mhppo_lanes_close(const mhppo_lanes *lanes, int32_t E, int64_t M, int32_t k, int32_t T, int32_t *len_out,
                      uint8_t *cut_out, void *stream);

/* The reward-to-go of the lanes over the wall-clock records rew float64 [T, M S] -> ret float32 [T, M S]:
 * lane-segment q = v S + i (v = e M + r) with pos[q] >= 0 scans column r S + i over t = t0[v] + L - 1 .. t0[v]
 * in float64, L = len[v], from G = (cut[v] && v_boot) ? (double)v_boot[r S + i] : 0, and stores float32;
 * every record in no used lane gets ret = 0 (a memset before the launch).  pos int64 [E M S] as
 * mhppo_bucket_plan writes it over N = E M; t0 / len int32 [E M] and cut uint8 [E M] as mhppo_lanes_close
 * leaves them (a lane whose t0 / len leave [0, T] is clamped into it); v_boot float32 [M S] or NULL.  One
 * thread per lane-segment, consecutive threads on consecutive columns.
 * MHPPO_EINVAL: E < 1, M < 0, S < 1, E M S > 2^31 - 1, T < 1, for M > 0 a NULL pointer other than v_boot. */
int mhppo_returns_scan_tm_lanes(const double *rew, float *ret, int64_t M, int32_t S, int32_t E, int32_t T,
                                double gamma, const int64_t *pos, const int32_t *t0, const int32_t *len,
                                const uint8_t *cut, const float *v_boot, void *stream);

/* mhppo_bucket_scatter_ragged over lanes: record (t0[v] + j, r S + i) of a lane-segment q = v S + i with
 * row0[q] >= 0 goes to row row0[q] + j of dst[bucket[q]], j < len[v]; nothing else is written.  row0 int64
 * / bucket int8 [E M S] as mhppo_ragged_plan / mhppo_bucket_plan write them over the E M lanes.  The lanes
 * of a stream must not overlap in time (mhppo_lanes_close's do not); the caller's buffers hold every row
 * row0[q] + len[v] - 1.  rew_sums[b] adds (double)(float)rew over bucket b's records in the fixed order of
 * mhppo_bucket_scatter_sums: the blocks are 64 columns x 16 steps of the records, so with E == 1 the sums
 * are mhppo_bucket_scatter_ragged's bit for bit.  work: mhppo_bucket_work_bytes(M S, T) bytes.
 * MHPPO_EINVAL: E < 1, M < 0, S < 1, E M S > 2^31 - 1, T < 1, dst NULL, for M > 0 any NULL pointer. */
int mhppo_bucket_scatter_lanes(const int64_t *row0, const int8_t *bucket, const int32_t *t0, const int32_t *len,
                               int64_t M, int32_t S, int32_t E, int32_t T, const float *obs_tm, const float *act_tm,
                               const float *logp_tm, const float *ret_tm, const double *rew_tm,
                               const mhppo_bucket_dst *dst, double *rew_sums, void *work, void *stream);

const char *mhppo_last_error(void);
const char *mhppo_version(void);

#ifdef __cplusplus
}
#endif
#endif
