"""GPU rollout collector: one PPO iteration's episodes for N envs at once.

Batched form of `Env_rollout.iterations_rand` (Coop-MH-PPO-scalable.py:357-517;
coop driver Coop-MH-PPO.ipynb cell 0): every env plays one 80-step episode;
the choice head is sampled once at t=0 (ped_traffic never changes, so
`need_new_d` is only true at the start); each step runs the
MFMA policy kernel and the fused sample+env-step kernel.  The per-step records are
written time-major, [t, env, slot] (each step's writes are one contiguous block
in HBM); RolloutBatch exposes them as [env, slot, t] views, and bucket_segments
gathers (env, slot) segments over t into the reference's episode-major,
car-major, time-ascending batch order.

Noise: in perf mode the standard normals (MVN eps) and the Categorical
uniforms come from Philox keyed by (seed, iteration) with counters built from
the GLOBAL env id, so a sharded run draws the same noise per env as a single
GPU.  In parity mode callers pass the reference's recorded draws instead.
"""
import ctypes
import os

import torch

from . import _lib
from .policy import noise_key

NF_C = 13
_CTR_STEP = 1 << 40  # counter stride between time steps (global env*slot index below it)
GAMMA = 0.99  # the reward-to-go's discount in bucket_segments (futur_rewards, :668-672): every bucketing path's


class RolloutBatch:
    """Views of one iteration's rollout buffers (all on the env's device).  With the compact
    record layout (rec_of set: the scalable env, whose absent car slots store no records) obs_c /
    act / logp / rew are gathered from the time-major records on first access, absent segments
    zero — a full copy, not a view: at config 4 (524 288 segments x 80 steps) obs_c alone is
    2.2 GB, and the gather needs about twice that in temporaries.  The product path never touches
    them (bucket_segments reads the *_tm records through rec_of); they are for tests and tools."""

    _REC = ("obs_c", "act", "logp", "rew")

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __getattr__(self, name):
        if name not in RolloutBatch._REC or self.__dict__.get("rec_of") is None:
            raise AttributeError(name)
        N, S, T = self.N, self.S, self.T
        ro = self.rec_of.long()
        x = getattr(self, name + "_tm").reshape(T, N * S, -1).index_select(1, ro.clamp_min(0))
        x = torch.where((ro >= 0).reshape(1, -1, 1), x, torch.zeros((), dtype=x.dtype, device=x.device))
        x = x.reshape(T, N, S, -1).permute(1, 2, 0, 3)
        v = x if name == "obs_c" else x[..., 0]
        self.__dict__[name] = v
        return v


# Envs per part below which the rollout runs as one chain (parts = 1): with fewer than ~256 waves of
# envs per part the launches are too small for two streams to gain anything
PART_MIN_ENVS = 16384


def default_parts(n_envs, valu_policy=False):
    """2 (two independent step chains on two streams, RolloutGPU.collect) for large env counts,
    else 1.  MHPPO_ROLLOUT_PARTS overrides (A/B)."""
    import os
    env = os.environ.get("MHPPO_ROLLOUT_PARTS")
    if env:
        return max(1, int(env))
    return 2 if (not valu_policy and n_envs >= 2 * PART_MIN_ENVS) else 1


def default_graph():
    """Replay the one-chain step loop from a captured HIP graph (RolloutGPU.collect) unless
    MHPPO_ROLLOUT_GRAPH=0; =2 also captures the two-stream parts loop (measured no faster at
    config 3: 64.5-65.2 us per step either way, profiles/r04_host/graph_parts_ab.txt)."""
    import os
    return {"0": 0, "2": 2}.get(os.environ.get("MHPPO_ROLLOUT_GRAPH", "1"), 1)


class EvalStats:
    """The streaming evaluation statistics' device state for one env handle (include/mhppo.h
    mhppo_eval_stats_*): begin() zeroes it, row(obs, t, T) consumes row t of the current episode
    of every env (obs float32 [N, obs_dim] on the env's device: the live pre-step observation, or
    a row of a recorded trajectory), fold() returns the float64 [MHPPO_EVS_N] sums.  Calls go to
    the env's device's current stream.  ValueError for a layout get_average rejects (4cars)."""

    def __init__(self, venv):
        from .stats import EVS_N, check_variant
        check_variant(venv.variant)
        self.venv = venv
        n = _lib.eval_stats_bytes(venv.handle)
        self.state = torch.empty((n + 7) // 8, dtype=torch.float64, device=venv.device)
        self.n_sums = EVS_N

    def _st(self):
        return _lib.stream_ptr(device=self.venv.device)

    def begin(self):
        _lib.eval_stats_begin(self.venv.handle, _lib.ptr(self.state), self._st())

    def row(self, obs, t, T):
        v = self.venv
        if (obs.dtype != torch.float32 or obs.device != v.device or tuple(obs.shape) != (v.n_envs, v.obs_dim)
                or not obs.is_contiguous()):
            raise ValueError(f"EvalStats.row takes a contiguous float32 [{v.n_envs}, {v.obs_dim}] on {v.device}")
        _lib.eval_stats_row(v.handle, _lib.ptr(obs), int(t), int(T), _lib.ptr(self.state), self._st())

    def fold(self):
        sums = torch.empty(self.n_sums, dtype=torch.float64, device=self.venv.device)
        _lib.eval_stats_fold(self.venv.handle, _lib.ptr(self.state), _lib.ptr(sums), self._st())
        return sums


class RolloutGPU:
    def __init__(self, venv, T=None, valu_policy=False, parts=None):
        if venv.variant == "4cars2":
            raise ValueError("4cars2 is an env-level variant only: the reference has no driver for it and its "
                             "PPO-driven followers earn no reward (Env_hybrid_multi_coop_4cars2.py:836-847)")
        self.venv = venv
        self.T = T or venv.max_episode
        N, S, P = venv.n_envs, venv.n_slots, venv.nb_ped
        self.N, self.S, self.P = N, S, P
        self.dc = _lib.lib().mhppo_choice_dim(venv.handle)
        dev = venv.device
        f32, f64, i32 = torch.float32, torch.float64, torch.int32
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.feat_d = z((N, S, P, self.dc), f32)
        self.probs_d = z((N, S, P, 2), f32)
        self.logp_d = z((N, S, P), f32)
        self.a_d = z((N, S, P), i32)
        self.closest = z((N, S), i32)
        self.feat_c = z((N, S, P, NF_C), f32)
        self.out_c = z((N, S, P), f32)
        self.obs = z((N, venv.obs_dim), f32)
        # time-major records [T, N, S(, 13)] (include/mhppo.h mhppo_rollout_bufs)
        self.obs_c = z((self.T, N, S, NF_C), f32)
        self.act = z((self.T, N, S), f32)
        self.logp = z((self.T, N, S), f32)
        self.rew = z((self.T, N, S), f64)
        self.ep_min = z((N, S), f64)
        self.exist = z((N, S), torch.uint8)
        self.eps = z((self.T, N, S), f32)
        self.u = z((N, S, P), f32)
        # the compact record layout (include/mhppo.h mhppo_rollout_bufs.rec_of) where car slots can
        # be absent (the scalable env): absent segments store no records, present ones are
        # contiguous (MHPPO_COMPACT_RECORDS=0: the identity layout)
        self.compact = venv.variant == "scalable" and os.environ.get("MHPPO_COMPACT_RECORDS", "1") != "0"
        self.rec_buf = z(N * S + N + 1, i32) if self.compact else None  # segment ranks | per-env prefix
        self.rec_of = self.rec_buf[:N * S] if self.compact else None
        self.parts = default_parts(N, valu_policy) if parts is None else int(parts)
        if self.parts > 1 and valu_policy:
            raise ValueError("parts > 1 runs the MFMA policy kernel only")
        # head-sorted policy rows (filled by mhppo_rollout_begin) + the parts' bounds in them
        self.rows = z(N * S * P + 2 + 2 * (self.parts + 1), i32)
        self.status = z(1, i32)  # NaN flags of the policy draws (mhppo_rollout_check)
        b = _lib.RolloutBufs()
        for name in ("feat_d", "probs_d", "logp_d", "a_d", "closest", "feat_c", "out_c", "obs", "obs_c", "act",
                     "logp", "rew", "ep_min", "exist", "rows", "status"):
            setattr(b, name, ctypes.c_void_p(getattr(self, name).data_ptr()))
        b.T = self.T
        b.rec_of = ctypes.c_void_p(self.rec_buf.data_ptr()) if self.compact else None
        # policy step on the VALU reference kernels instead of the MFMA one (bit-identical; tests, with
        # the test build of the library: MHPPO_LIB=tests/lib/libmhppo_test.so); "unsorted": the
        # one-lane-per-row kernel
        b.flags = {False: 0, True: _lib.MHPPO_ROLLOUT_VALU_POLICY,
                   "unsorted": _lib.MHPPO_ROLLOUT_VALU_POLICY | _lib.MHPPO_ROLLOUT_VALU_UNSORTED}[valu_policy]
        b.parts = self.parts
        self._bufs = b
        # captured one-chain step loops, keyed by what their launches bake in (collect)
        self._graphs = {}
        self._cap_stream = None  # the graph capture stream, on the env's device (created at first capture)
        self.use_graph = default_graph() if dev.type == "cuda" else 0
        # parts > 1: part p > 0 steps on its own stream (created once), part 0 on the caller's
        self._side = [torch.cuda.Stream(device=dev) for _ in range(self.parts - 1)] if dev.type == "cuda" else []

    def evaluate(self, actor_cross, actor_wait, actor_choice, episodes=1, choix=False):
        """Deterministic evaluation (Env_rollout.iterations :152-252): `episodes` consecutive
        episodes in every env (env e's episodes continue its own random stream).
        Returns the five tensors iterations returns, env-major (env 0's episodes first),
        on the env's device: obs [N*K*T, obs_dim], acts [N*K*T, S], rews_c [N*K*T, S]
        (float32), rews_d [saves, S], waiting [saves * P].  choix=True plays the scripted
        choix_test scenario (:629-633) after every reset (scalable env only)."""
        L = _lib.lib()
        venv, N, S, P, T = self.venv, self.N, self.S, self.P, self.T
        dev = venv.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        E = dict(obs=z((N, venv.obs_dim), torch.float32), a_d=z((N, S, P), torch.int32),
                 trig=z(N, torch.uint8), ep_min=z((N, S), torch.float64))
        hist = {k: [] for k in ("obs", "acts", "rews_c", "rews_d", "waiting", "saved")}
        mc, tc = actor_cross.mlp_desc()
        mw, tw = actor_wait.mlp_desc()
        md, td = actor_choice.mlp_desc()
        st = _lib.stream_ptr(device=venv.device)
        for _ in range(episodes):
            R = dict(obs_hist=z((T, N, venv.obs_dim), torch.float32), acts=z((T, N, S), torch.float32),
                     rews_c=z((T, N, S), torch.float32), rews_d=z((T, N, S), torch.float32),
                     waiting=z((T, N, P), torch.float32), saved=z((T, N), torch.uint8))
            b = _lib.EvalBufs()
            for k, v in list(E.items()) + list(R.items()):
                setattr(b, k, ctypes.c_void_p(v.data_ptr()))
            b.T = T
            _lib.check(L.mhppo_env_reset(venv.handle, _lib.ptr(E["obs"]), st))
            if choix:  # iterations(choix=True): choix_test + get_state (:170-172)
                _lib.check(L.mhppo_env_choix_test(venv.handle, _lib.ptr(E["obs"]), st))
            for t in range(T):
                _lib.check(L.mhppo_eval_step(venv.handle, ctypes.byref(mc), ctypes.byref(mw), ctypes.byref(md), t,
                                             ctypes.byref(b), st))
            hist["obs"].append(R["obs_hist"].transpose(0, 1))  # [N, T, od]
            for k in ("acts", "rews_c", "rews_d", "waiting", "saved"):
                hist[k].append(R[k].transpose(0, 1))
        cat = {k: torch.stack(v, 1) for k, v in hist.items()}  # [N, K, T, ...]
        saved = cat["saved"].reshape(-1).bool()
        return (cat["obs"].reshape(-1, venv.obs_dim), cat["acts"].reshape(-1, S), cat["rews_c"].reshape(-1, S),
                cat["rews_d"].reshape(-1, S)[saved], cat["waiting"].reshape(-1, P)[saved].reshape(-1))

    def evaluate_stats(self, actor_cross, actor_wait, actor_choice, episodes=1, choix=False):
        """evaluate() reduced on the device to get_average's sums (opt-in, beyond the reference):
        the same resets and steps in the same order — the env ends in the state evaluate(episodes)
        leaves it in — but no history is kept: each step's pre-step observation goes through
        mhppo_eval_stats_row into per-env accumulators, folded once at the end.  Memory is O(N)
        whatever `episodes` is; nothing is allocated per episode and nothing read back.
        Returns float64 [MHPPO_EVS_N] on the env's device (mhppo.stats.stats_from_sums makes the
        dict; the sums add across ranks).  Episodes are the true ones, N * episodes in all, also
        under choix=True, where get_average's equal-width runs merge them into one."""
        L = _lib.lib()
        venv, N, S, P, T = self.venv, self.N, self.S, self.P, self.T
        dev = venv.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        acc = EvalStats(venv)
        E = dict(obs=z((N, venv.obs_dim), torch.float32), a_d=z((N, S, P), torch.int32),
                 trig=z(N, torch.uint8), ep_min=z((N, S), torch.float64), saved=z((T, N), torch.uint8))
        b = _lib.EvalBufs()  # the histories stay NULL: mhppo_eval_step skips their stores
        for k, v in E.items():
            setattr(b, k, ctypes.c_void_p(v.data_ptr()))
        b.T = T
        mc, tc = actor_cross.mlp_desc()
        mw, tw = actor_wait.mlp_desc()
        md, td = actor_choice.mlp_desc()
        st = _lib.stream_ptr(device=dev)
        acc.begin()
        for _ in range(episodes):
            _lib.check(L.mhppo_env_reset(venv.handle, _lib.ptr(E["obs"]), st))
            if choix:
                _lib.check(L.mhppo_env_choix_test(venv.handle, _lib.ptr(E["obs"]), st))
            for t in range(T):
                acc.row(E["obs"], t, T)
                _lib.check(L.mhppo_eval_step(venv.handle, ctypes.byref(mc), ctypes.byref(mw), ctypes.byref(md), t,
                                             ctypes.byref(b), st))
        return acc.fold()

    def check(self):
        """Raise MhppoNaNError (a ValueError, as the reference's torch.distributions raise) if
        a NaN policy output was sampled since the last check.  Synchronises the stream."""
        _lib.check(_lib.lib().mhppo_rollout_check(ctypes.byref(self._bufs), _lib.stream_ptr(device=self.venv.device)))

    def draw_noise(self, seed, iteration):
        """Philox perf-mode noise for one iteration (global-env-id counters)."""
        L = _lib.lib()
        key = noise_key(seed, iteration)
        off = int(self.venv.cfg.env_id_offset)
        st = _lib.stream_ptr(device=self.venv.device)
        _lib.check(L.mhppo_philox_uniform(key, off * self.S * self.P, _lib.ptr(self.u), self.u.numel(), st))
        # step t's normals from counters (t + 1) * 2^40 + global (env, slot): one launch
        _lib.check(L.mhppo_philox_normal_2d(key, _CTR_STEP + off * self.S, _CTR_STEP, _lib.ptr(self.eps), self.T,
                                            self.eps[0].numel(), st))

    def _step_loop(self, L, mx, mw, st, step_events):
        """The T steps as one chain on stream `st`: policy + env step."""
        for t in range(self.T):
            if self.P == 1:  # features straight into the step's record (include/mhppo.h)
                self._bufs.feat_c = self.obs_c[t].data_ptr()
            _lib.check(L.mhppo_rollout_policy(self.venv.handle, ctypes.byref(mx), ctypes.byref(mw),
                                              ctypes.byref(self._bufs), st))
            if step_events is not None:  # HIP events bracketing the env-step kernel on this stream
                step_events[t][0].record()
            _lib.check(L.mhppo_rollout_sample_env(self.venv.handle, _lib.ptr(self.eps[t]), t,
                                                  ctypes.byref(self._bufs), st))
            if step_events is not None:
                step_events[t][1].record()

    def _parts_loop(self, L, mx, mw, nparts, main):
        """Two-stream rollout: the parts' step chains (policy -> env step -> policy ...) are
        independent, so one part's policy MFMA work fills the CUs that another part's
        latency-bound env step leaves idle (one wave per SIMD, the launch lasting as long as its
        slowest wave).  Part 0 on `main`, part p > 0 on side stream p - 1, forked from and joined
        back to `main`.  The same kernels and results as the one-chain loop."""
        forked = torch.cuda.Event()
        forked.record(main)
        for side in self._side[:nparts - 1]:
            side.wait_event(forked)
        streams = [main.cuda_stream] + [side.cuda_stream for side in self._side[:nparts - 1]]
        for t in range(self.T):
            if self.P == 1:  # features straight into the step's record (include/mhppo.h)
                self._bufs.feat_c = self.obs_c[t].data_ptr()
            for part, sp in enumerate(streams):
                _lib.check(L.mhppo_rollout_policy_part(self.venv.handle, ctypes.byref(mx), ctypes.byref(mw),
                                                       ctypes.byref(self._bufs), part, sp))
                _lib.check(L.mhppo_rollout_sample_env_part(self.venv.handle, _lib.ptr(self.eps[t]), t,
                                                           ctypes.byref(self._bufs), part, sp))
        for side in self._side[:nparts - 1]:
            main.wait_stream(side)

    def collect(self, actor_cross, actor_wait, actor_choice, seed=0, iteration=0, forced_choice=None,
                eps_tape=None, step_events=None, parts=None, graph=None):
        """Run one episode in every env.  forced_choice int32 [N,S,P] / eps_tape float32 [T,N,S]
        replay recorded draws (parity mode); otherwise Philox noise is drawn.  parts: 1 forces the
        one-chain loop for this call (default: self.parts); step_events implies it.  step_events
        brackets each step's env-step launch.  graph: replay the step loop
        from a captured HIP graph (default: self.use_graph; pass False while mhppo_kernel_timing is
        on — graph nodes carry no timing events)."""
        L = _lib.lib()
        nparts = self.parts if parts is None else min(int(parts), self.parts)
        if step_events is not None:
            nparts = 1
        self._bufs.parts = nparts
        if forced_choice is None or eps_tape is None:
            self.draw_noise(seed, iteration)
        if eps_tape is not None:
            self.eps.copy_(eps_tape.to(self.eps.device, torch.float32))
        fa = None
        if forced_choice is not None:
            fa = forced_choice.to(self.a_d.device, torch.int32).contiguous()
        mc, tc = actor_choice.mlp_desc()
        mx, tx = actor_cross.mlp_desc()
        mw, tw = actor_wait.mlp_desc()
        dev = self.venv.device
        st = _lib.stream_ptr(device=dev)
        _lib.check(L.mhppo_rollout_begin(self.venv.handle, ctypes.byref(mc), _lib.ptr(self.u), _lib.ptr(fa),
                                         ctypes.byref(self._bufs), st))
        if graph is None:  # the default: the one-chain loop (and with MHPPO_ROLLOUT_GRAPH=2 the parts loop)
            graph = bool(self.use_graph) and (nparts == 1 or self.use_graph == 2)
        graph = bool(graph) and dev.type == "cuda"
        if step_events is None and graph:
            # The step loop's launches (one chain: 160; parts: 160 per part on their
            # streams, forked from and joined back to the capture stream) as one captured HIP
            # graph, replayed: the same kernels and arguments (the pointers, step indices and the
            # actors' mean / std are baked into the graph's nodes and key it), without the
            # per-launch host work — which at small N is the step's time, and at large N keeps the
            # host from queueing the bucketing until the rollout has nearly finished.
            # Capture and replay with the env's device current and on a capture stream OF that
            # device: torch.cuda.graph's default capture stream is created once, on whichever
            # device was current at its first use, and a launch on another device's stream would
            # run eagerly outside the capture (an empty graph, replayed silently).  The replay
            # goes to dev's current stream, ordered after mhppo_rollout_begin above.
            key = (nparts, mx.packed, mw.packed, mx.mean, mx.std, mw.mean, mw.std)
            with torch.cuda.device(dev):
                g = self._graphs.get(key)
                if g is None:
                    if self._cap_stream is None:
                        self._cap_stream = torch.cuda.Stream(device=dev)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=self._cap_stream):
                        cap = torch.cuda.current_stream(dev)
                        assert cap == self._cap_stream, "graph capture must run on the env's device"
                        if nparts == 1:
                            self._step_loop(L, mx, mw, cap.cuda_stream, None)
                        else:
                            self._parts_loop(L, mx, mw, nparts, cap)
                    if len(self._graphs) > 8:
                        self._graphs.clear()
                    self._graphs[key] = g
                g.replay()
        elif nparts == 1:
            self._step_loop(L, mx, mw, st, step_events)
        else:
            self._parts_loop(L, mx, mw, nparts, torch.cuda.current_stream(dev))
        del tc, tx, tw, fa  # keep the packed weights alive until the launches are queued
        # obs_c/act/logp/rew: [N, S, T(, 13)] views of the time-major buffers (*_tm)
        views = {} if self.compact else dict(obs_c=self.obs_c.permute(1, 2, 0, 3), act=self.act.permute(1, 2, 0),
                                             logp=self.logp.permute(1, 2, 0), rew=self.rew.permute(1, 2, 0))
        return RolloutBatch(feat_d=self.feat_d, probs_d=self.probs_d, logp_d=self.logp_d, a_d=self.a_d,
                            closest=self.closest, **views, obs_c_tm=self.obs_c,
                            act_tm=self.act, logp_tm=self.logp, rew_tm=self.rew, ep_min=self.ep_min, rec_of=self.rec_of,
                            exist=self.exist, N=self.N, S=self.S, P=self.P, T=self.T)


def _check_len_rec(len_rec, B, dev, who):
    if (not torch.is_tensor(len_rec) or len_rec.dtype != torch.int32 or len_rec.numel() != B or len_rec.device != dev):
        raise ValueError(f"{who}: len_rec is an int32 [{B}] tensor on the records' device")
    return len_rec.reshape(B).contiguous()


def _check_v_boot(v_boot, B, dev, who):
    if (not torch.is_tensor(v_boot) or v_boot.dtype != torch.float32 or v_boot.numel() != B or v_boot.device != dev):
        raise ValueError(f"{who}: v_boot is a float32 [{B}] tensor on the records' device")
    return v_boot.reshape(B).contiguous()


def returns_scan_tm(rew_tm, gamma=GAMMA, len_rec=None, v_boot=None):
    """futur_rewards over time-major records: rew float64 [T, ...] (one segment per column)
    -> float32 [T, ...].  len_rec int32 [B] (early episode ends, mhppo_returns_scan_tm_len): column b
    has len_rec[b] steps (clamped to [0, T]); its scan starts from G = 0 at its last step -- the early
    end is terminal, as the time limit is -- and the return is 0 from there on.  v_boot float32 [B]
    (truncation bootstrap, mhppo_returns_scan_tm_boot): the scan of column b starts from G = v_boot[b]
    instead, ret[L - 1] = float32(rew[L - 1] + gamma float64(v_boot)); a column of no steps stays 0."""
    T = rew_tm.shape[0]
    r = rew_tm.reshape(T, -1).contiguous()
    out = torch.empty(r.shape, dtype=torch.float32, device=rew_tm.device)
    if len_rec is not None:
        len_rec = _check_len_rec(len_rec, r.shape[1], rew_tm.device, "returns_scan_tm")
    if v_boot is not None:
        v_boot = _check_v_boot(v_boot, r.shape[1], rew_tm.device, "returns_scan_tm")
    if rew_tm.device.type != "cuda":  # the torch path's CPU form: G_t = r_t + gamma G_{t+1} in float64
        g = torch.zeros_like(r[0])
        if v_boot is not None:
            last = (torch.full_like(v_boot, T, dtype=torch.int32) if len_rec is None else len_rec.clamp(0, T)) - 1
        for t in range(T - 1, -1, -1):
            if v_boot is not None:  # the specification of the native scan's start
                g = torch.where(last == t, v_boot.double(), g)
            g = r[t] + gamma * g
            if len_rec is not None:  # the specification of the native scan's cut
                g = torch.where(t < len_rec, g, torch.zeros_like(g))
            out[t] = g.float()
        return out.reshape(rew_tm.shape)
    with torch.cuda.device(rew_tm.device):  # the records' device and its current stream
        st = _lib.stream_ptr(device=rew_tm.device)
        if v_boot is not None:
            _lib.check(_lib.lib().mhppo_returns_scan_tm_boot(_lib.ptr(r), _lib.ptr(out), r.shape[1], T, gamma,
                                                             _lib.ptr(len_rec), _lib.ptr(v_boot), st))
        elif len_rec is None:
            _lib.check(_lib.lib().mhppo_returns_scan_tm(_lib.ptr(r), _lib.ptr(out), r.shape[1], T, gamma, st))
        else:
            _lib.check(_lib.lib().mhppo_returns_scan_tm_len(_lib.ptr(r), _lib.ptr(out), r.shape[1], T, gamma,
                                                            _lib.ptr(len_rec), st))
    return out.reshape(rew_tm.shape)


def returns_scan(rew, gamma=0.99):
    """futur_rewards (:658-684): float64 reverse discounted scan per [.., T] row -> float32."""
    T = rew.shape[-1]
    r = rew.reshape(-1, T).contiguous()
    out = torch.empty(r.shape, dtype=torch.float32, device=rew.device)
    with torch.cuda.device(rew.device):
        _lib.check(_lib.lib().mhppo_returns_scan(_lib.ptr(r), _lib.ptr(out), r.shape[0], T, gamma,
                                                 _lib.stream_ptr(device=rew.device)))
    return out.reshape(rew.shape)


def gae_targets_torch(rew_tm, v_tm, gamma, lam, out_dtype=torch.float32, len_rec=None, v_boot=None):
    """lambda-return targets R_t = A_t + V_t over time-major records in float64 torch ops (any
    device): the executable specification of mhppo_gae_tm's recurrence (include/mhppo.h, the
    same operation order) and the CPU path.  rew_tm [T, ...] float64, v_tm [T, ...] -> float32
    (out_dtype=torch.float64: the values before the cast).
    A_t = sum_k (gamma lam)^k delta_{t+k}, delta_t = r_t + gamma V_{t+1} - V_t, V_T = 0: no
    bootstrap past the last step (the episode's time limit is terminal, as in futur_rewards).
    len_rec int32 (one per column, mhppo_gae_tm_len): column b has len_rec[b] steps; its recurrence
    starts from A = nv = 0 at its last step and the target is 0 from there on.
    v_boot float32 (one per column, mhppo_gae_tm_boot; needs len_rec): the recurrence of column b starts
    from nv = v_boot[b], the value after its last step, instead of 0 (a truncated episode)."""
    if rew_tm.shape != v_tm.shape:
        raise ValueError("gae_targets_torch: rew_tm and v_tm differ in shape")
    r, v = rew_tm.double(), v_tm.double()
    if v_boot is not None and len_rec is None:
        raise ValueError("gae_targets_torch: v_boot needs len_rec")
    if len_rec is not None:
        len_rec = _check_len_rec(len_rec, r[0].numel(), r.device, "gae_targets_torch").reshape(r[0].shape)
    if v_boot is not None:
        v_boot = _check_v_boot(v_boot, r[0].numel(), r.device, "gae_targets_torch").reshape(r[0].shape).double()
        last = len_rec.clamp(0, r.shape[0]) - 1
    out = torch.empty(r.shape, dtype=out_dtype, device=r.device)
    c = float(gamma) * float(lam)
    A = torch.zeros_like(r[0])
    nv = torch.zeros_like(r[0])
    zero = torch.zeros_like(r[0])
    for t in range(r.shape[0] - 1, -1, -1):
        if v_boot is not None:
            nv = torch.where(last == t, v_boot, nv)
        d = (r[t] + gamma * nv) - v[t]
        A = d + c * A
        R = A + v[t]
        nv = v[t]
        if len_rec is not None:
            live = t < len_rec
            A, R, nv = torch.where(live, A, zero), torch.where(live, R, zero), torch.where(live, nv, zero)
        out[t] = R.to(out_dtype)
    return out


def gae_targets_tm(obs_tm, rew_tm, critic0, critic1=None, pos=None, bucket=None, gamma=0.99, lam=0.95,
                   want_value=False, len_rec=None, v_boot=None):
    """mhppo_gae_tm: the critics' forward and the lambda-return scan over time-major records in one
    launch.  obs_tm float32 [T, ..., n_in], rew_tm float64 [T, ...] (B records per step) on the
    critics' GPU; pos int64 [B] / bucket int8 [B] as mhppo_bucket_plan writes them (record b is used
    iff pos[b] >= 0, with critic0 / critic1 for bucket 0 / 1), or pos=None: every record, critic0.
    Returns ret float32 shaped like rew_tm (0 for unused records), with want_value also the critic
    outputs the scan used.  V is forward_rows' bit for bit; the recurrence is gae_targets_torch's.
    len_rec int32 [B] (early episode ends, mhppo_gae_tm_len): record b has len_rec[b] steps; ret and
    the values are 0 at and beyond them.  v_boot float32 [B] (truncation bootstrap, mhppo_gae_tm_boot;
    needs len_rec): record b's recurrence starts from nv = v_boot[b]."""
    T = rew_tm.shape[0]
    dev = rew_tm.device
    B = rew_tm[0].numel()
    r = rew_tm.reshape(T, B).contiguous()
    x = obs_tm.reshape(T, B, obs_tm.shape[-1]).contiguous()
    if x.dtype != torch.float32 or r.dtype != torch.float64 or x.device != dev or dev.type != "cuda":
        raise ValueError("gae_targets_tm takes float32 observations and float64 rewards on one GPU")
    if x.shape[2] != critic0.n_in:
        raise ValueError(f"gae_targets_tm: observations of width {x.shape[2]} for a critic of {critic0.n_in} inputs")
    if pos is not None:
        if critic1 is None or bucket is None:
            raise ValueError("gae_targets_tm: pos needs bucket and critic1")
        if (pos.dtype != torch.int64 or bucket.dtype != torch.int8 or pos.numel() != B or bucket.numel() != B
                or pos.device != dev or bucket.device != dev):
            raise ValueError(f"gae_targets_tm: pos int64 [{B}] and bucket int8 [{B}] on the records' device")
        pos, bucket = pos.contiguous(), bucket.contiguous()
    else:
        bucket = None
    if len_rec is not None:
        len_rec = _check_len_rec(len_rec, B, dev, "gae_targets_tm")
    if v_boot is not None:
        if len_rec is None:
            raise ValueError("gae_targets_tm: v_boot needs len_rec")
        v_boot = _check_v_boot(v_boot, B, dev, "gae_targets_tm")
    ret = torch.empty((T, B), dtype=torch.float32, device=dev)
    val = torch.empty((T, B), dtype=torch.float32, device=dev) if want_value else None
    d0, keep0 = critic0.mlp_desc()
    d1, keep1 = critic1.mlp_desc() if critic1 is not None else (None, None)
    if keep0.device != dev or (keep1 is not None and keep1.device != dev):
        raise ValueError("gae_targets_tm: the critics must live on the records' device")
    with torch.cuda.device(dev):
        args = (ctypes.byref(d0), ctypes.byref(d1) if d1 is not None else None, _lib.ptr(x), _lib.ptr(r),
                _lib.ptr(pos), _lib.ptr(bucket), B, T, float(gamma), float(lam), _lib.ptr(ret), _lib.ptr(val))
        if v_boot is not None:
            _lib.gae_tm_boot(*args, _lib.ptr(len_rec), _lib.ptr(v_boot), _lib.stream_ptr(device=dev))
        elif len_rec is None:
            _lib.gae_tm(*args, _lib.stream_ptr(device=dev))
        else:
            _lib.gae_tm_len(*args, _lib.ptr(len_rec), _lib.stream_ptr(device=dev))
    ret = ret.reshape(rew_tm.shape)
    return (ret, val.reshape(rew_tm.shape)) if want_value else ret


NAN_STATUS_MSG = {1: "Categorical probs of the choice actor, :409",
                  2: "MultivariateNormal loc of the continuous actors, :451"}


def raise_if_nan_status(st):
    """The host side of mhppo_rollout_check for a status word already read back: raise
    MhppoNaNError (a ValueError, as the reference's torch.distributions raise) when set."""
    st = int(st)
    if st:
        what = "; ".join(m for b, m in NAN_STATUS_MSG.items() if st & b)
        raise _lib.MhppoNaNError(f"NaN policy output sampled ({what}): the reference raises ValueError here")


def bucket_segments(batch, fix_bucket=False, status=None, gae=None, boot=None):
    """Split (env, slot) episode segments into the reference's cross/wait/choice batches.
    fix_bucket=True (opt-in bug fix) buckets car i by ITS closest
    pedestrian's decision action_d[i*P + closest_i] instead of the flat action_d[i].

    Bucket rule (:489-507): only existing cars (scalable driver); cross when
    action_d[i] <= 0 where action_d is the per-(car, ped) array indexed by the CAR
    index i.  Choice sample per existing car: the closest pedestrian's
    features, action and log-prob, reward = episodic min of reward_light.

    One host synchronisation: the three bucket sizes (and, when `status` -- the rollout's
    NaN-flag word, int32 [1] on the device -- is given, that word, raised on as
    RolloutGPU.check would) come back in one read.

    On the GPU the plan (positions, choice batch, sizes, counts, reward sums) is one native pass,
    mhppo_bucket_plan, and the scatter also folds the cross / wait reward sums
    (bucket_segments_native); CPU tensors take the torch path (bucket_segments_torch), which
    also runs on CUDA tensors: it is the native pass's reference.  The native path adds
    choice["rew_sums"]: float64 [3] on the device, the sums over the cross rows' / the wait
    rows' float32 rewards and the choice batch's `ret` (Algo_PPO.train's reward curves).

    gae = (critic_cross, critic_wait, gamma, lam) (opt-in, Algo_PPO(gae_lambda=...)): the cross /
    wait buckets' `ret` are the GAE(lam) lambda-returns A_t + V_t under those critics instead of the
    reward-to-go (gae_targets_tm on the GPU: one launch with the plan's pos / bucket, queued before
    the host read, in place of the returns scan; gae_targets_torch on the torch path).  The choice
    batch keeps its episodic-min target: it is a one-step decision.

    A batch with early episode ends (batch.len set: ExternalRollout(early_end=True)) takes the ragged
    path, bucket_segments_ragged_native / _torch: a segment of a stream that ended after L steps owns L
    rows, the dicts gain `rows`, and both paths provide choice["rew_sums"].

    boot = (critic_cross, critic_wait) (opt-in, ragged batches only: ExternalRollout(bootstrap=True)): a
    segment whose episode was truncated (batch.trunc at a done, batch.cut_truncates at the cut) starts
    its reward-to-go or GAE scan from V(s_L) under its bucket's critic instead of 0 (boot_values).

    A batch with auto-reset lanes (batch.lanes = E: ExternalRollout(auto_reset=E)) takes
    bucket_segments_lanes_native / _torch: one segment per (lane, slot), rows in lane-segment order, the
    dicts' keys those of the ragged path.  gae with such a batch raises (the lambda-return kernel takes
    one length per column); boot bootstraps the lanes cut when the batch was taken.
    """
    if getattr(batch, "lanes", None) is not None:  # auto-reset: several episodes per stream
        if batch.a_d.device.type == "cuda":
            return bucket_segments_lanes_native(batch, fix_bucket, status, gae=gae, boot=boot)
        return bucket_segments_lanes_torch(batch, fix_bucket, status, gae=gae, boot=boot)
    if getattr(batch, "len", None) is not None:  # early episode ends: ragged buckets
        if batch.a_d.device.type == "cuda":
            return bucket_segments_ragged_native(batch, fix_bucket, status, gae=gae, boot=boot)
        return bucket_segments_ragged_torch(batch, fix_bucket, status, gae=gae, boot=boot)
    if boot is not None:
        raise ValueError("bucket_segments: boot needs a batch with early episode ends (batch.len)")
    if batch.a_d.device.type == "cuda":
        return bucket_segments_native(batch, fix_bucket, status, gae=gae)
    return bucket_segments_torch(batch, fix_bucket, status, gae=gae)


def bucket_plan(batch, fix_bucket=False, status=None):
    """mhppo_bucket_plan on a rollout batch (CUDA).  Returns the raw device outputs: pos int64 [NS]
    and bucket int8 [NS] (per record with the compact layout), the choice batch in NS-row buffers
    (obs / act / logp / ret), info (int64 [9]: n_cross, n_wait, n_all, status, then the bits of
    five float64: the two choice action counts and the three reward sums) and the scratch."""
    N, S, P, T = batch.N, batch.S, batch.P, batch.T
    NS = N * S
    dev = batch.a_d.device
    L = _lib.lib()
    dc = batch.feat_d.shape[-1]
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    src = dict(a_d=batch.a_d.to(torch.int32), closest=batch.closest.to(torch.int32), exist=batch.exist.to(torch.uint8),
               ep_min=batch.ep_min.to(torch.float64), feat_d=batch.feat_d.to(torch.float32),
               logp_d=batch.logp_d.to(torch.float32))
    src = {k: v.contiguous() for k, v in src.items()}
    rec_of = getattr(batch, "rec_of", None)
    if rec_of is not None:
        rec_of = rec_of.to(torch.int32).contiguous()
    out = dict(pos=e(NS, torch.int64), bucket=e(NS, torch.int8), obs=e((NS, dc), torch.float32),
               act=e(NS, torch.int32), logp=e(NS, torch.float32), ret=e(NS, torch.float32), info=e(9, torch.int64),
               work=e(max(1, int(L.mhppo_bucket_work_bytes(NS, T)) // 8), torch.float64))
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(L.mhppo_bucket_plan(N, S, P, dc, p(src["a_d"]), p(src["closest"]), p(src["exist"]), p(rec_of),
                                       p(src["ep_min"]), p(src["feat_d"]), p(src["logp_d"]), int(bool(fix_bucket)),
                                       p(status), p(out["pos"]), p(out["bucket"]), p(out["obs"]), p(out["act"]),
                                       p(out["logp"]), p(out["ret"]), p(out["info"]), p(out["work"]),
                                       _lib.stream_ptr(device=dev)))
    return out


def bucket_segments_native(batch, fix_bucket=False, status=None, gae=None):
    """bucket_segments on the GPU: the returns scan and mhppo_bucket_plan, then ONE scatter of both
    buckets into a shared buffer of NS + 3 segments that also folds the cross / wait reward sums
    (mhppo_bucket_scatter_sums).  The one host read comes right after the plan, before the scatter
    is queued (it needs no sizes): the update's host-side preparation then runs while the scatter
    does, instead of in an idle gap before the first critic launch.  (The returns stay their own
    pass: computed inside the scatter, by one wave per 64-segment block, the iteration was 1.1 ms
    slower at config 3)  With gae the returns scan is replaced by
    mhppo_gae_tm, queued after the plan (it takes the plan's pos / bucket) and before the read."""
    N, S, P, T = batch.N, batch.S, batch.P, batch.T
    NS = N * S
    dev = batch.a_d.device
    L = _lib.lib()
    if gae is None:
        ret_tm = returns_scan_tm(batch.rew_tm)  # [T, N, S]
        plan = bucket_plan(batch, fix_bucket, status)
    else:
        critic_cross, critic_wait, gamma, lam = gae
        plan = bucket_plan(batch, fix_bucket, status)
        ret_tm = gae_targets_tm(batch.obs_c_tm, batch.rew_tm, critic_cross, critic_wait, plan["pos"], plan["bucket"],
                                gamma, lam)
    info = plan["info"]
    n = NS + 3
    both = dict(obs=torch.empty(n * T, NF_C, dtype=torch.float32, device=dev),
                act=torch.empty(n * T, dtype=torch.float32, device=dev),
                logp=torch.empty(n * T, dtype=torch.float32, device=dev),
                ret=torch.empty(n * T, dtype=torch.float32, device=dev),
                rew=torch.empty(n * T, dtype=torch.float64, device=dev))
    one = _lib.BucketDst(*[both[k].data_ptr() for k in ("obs", "act", "logp", "ret", "rew")])
    dst = (_lib.BucketDst * 2)(one, one)  # cross and wait rows share the buffer (bucket[] keys the sums)
    srcs = [x.contiguous() for x in (batch.obs_c_tm, batch.act_tm, batch.logp_tm)]
    rew_tm = batch.rew_tm.contiguous()
    p = _lib.ptr
    args = (p(plan["pos"]), p(plan["bucket"]), NS, T, *[p(x) for x in srcs], p(ret_tm), p(rew_tm), dst,
            ctypes.c_void_p(info.data_ptr() + 48), p(plan["work"]), _lib.stream_ptr(device=dev))
    n_cross, n_wait, n_all, st = info[:4].tolist()  # the one host read
    if status is not None:
        if st:
            status.zero_()
        raise_if_nan_status(st)
    with torch.cuda.device(dev):
        _lib.check(L.mhppo_bucket_scatter_sums(*args))
    c0 = (n_cross + 3) // 4 * 4  # = w0
    cross_r = {k: both[k][:n_cross * T] for k in ("obs", "act", "logp", "ret", "rew")}
    wait_r = {k: both[k][c0 * T:(c0 + n_wait) * T] for k in ("obs", "act", "logp", "ret", "rew")}
    cross_r["n_seg"], wait_r["n_seg"] = n_cross, n_wait
    choice = {k: plan[k][:n_all] for k in ("obs", "act", "logp", "ret")}
    choice["n_seg"] = n_all
    f64 = info[4:9].view(torch.float64)
    choice["counts"] = f64[0:2]  # float64 [2] on the device: (act == 0).sum(), (act == 1).sum()
    choice["rew_sums"] = f64[2:5]
    return cross_r, wait_r, choice


def bucket_segments_torch(batch, fix_bucket=False, status=None, plan_out=None, gae=None):
    """bucket_segments with torch ops (any device): the CPU path, and the reference the native
    plan is tested against.  The segment lists are built with nonzero_static at NS rows, so
    everything is queued before the one host read.  plan_out: a dict that receives the scatter's
    `pos` (per record with the compact layout) and the `wait` segment mask (tests).  With gae the
    buckets' `ret` come from gae_targets_torch with V = critic(obs) (torch's forward) per bucket."""
    N, S, P, T = batch.N, batch.S, batch.P, batch.T
    exist, cross, wait = _segment_masks(batch, fix_bucket)
    NS = N * S
    # Everything is queued before the one host sync, so the GPU runs it while the host waits for
    # the sizes: the returns scan; each segment's bucket position (its rank among its bucket's
    # segments in (env, slot) order = the nonzero order); the bucket scatter into buffers with
    # room for every segment; the choice batch gathered over all segment slots (existing ones
    # first: nonzero_static pads with slot 0); the choice action counts.  After the sync the
    # batches are leading views of those buffers.
    # Both buckets share ONE buffer of NS + 3 segments (not one of NS each: that doubled the
    # bucketing's peak memory): cross segments from slot 0, wait segments from slot w0 = the cross
    # count rounded up to a multiple of 4, computed on the device, so the wait bucket's observation
    # rows start 16-byte aligned at any T (the train kernels' LDS-DMA rows; 4 T 52 B = 16 T 13 B).
    if gae is None:
        ret = returns_scan_tm(batch.rew_tm)  # [T, N, S]
    else:  # the buckets' ret are computed from the scattered rows below
        ret = torch.zeros(batch.rew_tm.shape, dtype=torch.float32, device=batch.rew_tm.device)
    cc, cw = torch.cumsum(cross, 0), torch.cumsum(wait, 0)
    w0 = torch.div(cc[-1] + 3, 4, rounding_mode="floor") * 4
    pos = torch.where(cross, cc - 1, torch.where(wait, w0 + cw - 1, -1))
    bucket = torch.zeros(NS, dtype=torch.int8, device=pos.device)
    rec_of = getattr(batch, "rec_of", None)
    if rec_of is not None:  # the compact layout: the scatter's positions are per record
        idx = torch.where(rec_of >= 0, rec_of, NS).long()
        pos = torch.full((NS + 1,), -1, dtype=pos.dtype, device=pos.device).scatter_(0, idx, pos)[:NS]
    if plan_out is not None:
        plan_out.update(pos=pos, wait=wait)
    (both,) = scatter_positions(pos, bucket, (NS + 3,), NS, T, batch.obs_c_tm, batch.act_tm, batch.logp_tm, ret,
                                batch.rew_tm)
    choice, counts = _choice_torch(batch, exist)
    sizes = [cc[-1], cw[-1], exist.sum()]
    if status is not None:
        sizes.append(status.reshape(-1)[0].to(torch.int64))
    sizes = torch.stack(sizes).tolist()
    if status is not None:
        if sizes[3]:
            status.zero_()
        raise_if_nan_status(sizes[3])
    n_cross, n_wait, n_all = sizes[:3]
    c0 = (n_cross + 3) // 4 * 4  # = w0
    cross_r = {k: both[k][:n_cross * T] for k in ("obs", "act", "logp", "ret", "rew")}
    wait_r = {k: both[k][c0 * T:(c0 + n_wait) * T] for k in ("obs", "act", "logp", "ret", "rew")}
    cross_r["n_seg"], wait_r["n_seg"] = n_cross, n_wait
    if gae is not None:
        for b, critic in ((cross_r, gae[0]), (wait_r, gae[1])):
            n = b["ret"].numel() // T
            with torch.no_grad():
                v = critic(b["obs"]).reshape(n, T)
            b["ret"] = gae_targets_torch(b["rew"].reshape(n, T).t(), v.t(), gae[2], gae[3]).t().reshape(-1)
    choice = {k: v[:n_all] for k, v in choice.items()}
    choice["n_seg"] = n_all
    choice["counts"] = counts  # float64 [2] on the device: (act == 0).sum(), (act == 1).sum()
    return cross_r, wait_r, choice


def _segment_masks(batch, fix_bucket):
    """The bucket rule in torch ops (bucket_segments): exist, cross, wait as bool [NS]."""
    N, S, P = batch.N, batch.S, batch.P
    a_flat = batch.a_d.reshape(N, S * P)
    if fix_bucket:
        a_car = batch.a_d.reshape(N, S, P).gather(2, batch.closest.reshape(N, S, 1).long()).reshape(N, S)
        action_d_i = 2 * a_car.to(torch.int32) - 1
    else:
        action_d_i = 2 * a_flat[:, :S].to(torch.int32) - 1  # action_d[i], i < S
    exist = batch.exist.bool().reshape(-1)
    cross = exist & (action_d_i <= 0).reshape(-1)
    wait = exist & (action_d_i > 0).reshape(-1)
    return exist, cross, wait


def _choice_torch(batch, exist):
    """The choice batch gathered over all NS segment slots (existing ones first: nonzero_static pads
    with slot 0) and the choice action counts, float64 [2], in torch ops: nothing is read back."""
    NS, P = batch.N * batch.S, batch.P
    seg_all = torch.nonzero_static(exist, size=NS, fill_value=0).squeeze(1)
    cl = batch.closest.reshape(NS).long().index_select(0, seg_all)
    base = seg_all * P + cl
    dc = batch.feat_d.shape[-1]
    a_sel = batch.a_d.reshape(-1).index_select(0, base)
    choice = dict(
        obs=batch.feat_d.reshape(NS * P, dc).index_select(0, base),
        act=a_sel,
        logp=batch.logp_d.reshape(-1).index_select(0, base),
        ret=batch.ep_min.reshape(-1).index_select(0, seg_all).float(),
    )
    a_car = batch.a_d.reshape(NS, P).gather(1, batch.closest.reshape(NS, 1).long()).reshape(-1)
    counts = torch.stack([(exist & (a_car == 0)).sum(), (exist & (a_car == 1)).sum()]).to(torch.float64)
    return choice, counts


def _ragged_steps(batch):
    """(len, k) of a batch with early episode ends, checked."""
    N, T = batch.N, batch.T
    k = int(getattr(batch, "steps", T))
    ln = batch.len
    if not 1 <= k <= T:
        raise ValueError(f"a ragged batch has 1 <= steps <= T = {T} recorded steps, not {k}")
    if not torch.is_tensor(ln) or ln.dtype != torch.int32 or ln.numel() != N or ln.device != batch.a_d.device:
        raise ValueError(f"a ragged batch's len is an int32 [{N}] tensor on the batch's device")
    return ln.reshape(N).contiguous(), k


def ragged_plan_torch(pos, bucket, rec_of, len, M, S, k):
    """mhppo_ragged_plan in torch ops (any device): its executable specification.  pos int64 [M S] /
    bucket int8 [M S] per record column, rec_of int32 [M S] or None, len int32 [M], k recorded steps
    -> (row0 int64 [M S], len_rec int32 [M S], info int64 [2] = rows_cross, rows_wait).  Nothing is
    read back."""
    NS = M * S
    k = int(k)
    if k < 1:
        raise ValueError("ragged_plan_torch: k < 1")
    ln = len.reshape(M).to(torch.int64)
    eff = torch.where((ln <= 0) | (ln > k), torch.full_like(ln, k), ln)  # 0: still running, cut at k
    seg_len = eff.repeat_interleave(S)  # per segment: the S slots of a stream share its length
    if rec_of is None:
        len_rec = seg_len
    else:  # column rec_of[s] holds segment s's record; columns without a record get 0
        idx = torch.where(rec_of[:NS] >= 0, rec_of[:NS], NS).long()
        len_rec = torch.zeros(NS + 1, dtype=torch.int64, device=ln.device).scatter_(0, idx, seg_len)[:NS]
    used = pos >= 0
    m0, m1 = used & (bucket == 0), used & (bucket != 0)
    l0, l1 = len_rec * m0, len_rec * m1
    c0, c1 = torch.cumsum(l0, 0), torch.cumsum(l1, 0)
    zero = torch.zeros(1, dtype=torch.int64, device=ln.device)
    rows_cross, rows_wait = (c0[-1:], c1[-1:]) if NS else (zero, zero)
    w0 = torch.div(rows_cross + 3, 4, rounding_mode="floor") * 4
    row0 = torch.where(m0, c0 - l0, torch.where(m1, w0 + c1 - l1, torch.full_like(c0, -1)))
    return row0, len_rec.to(torch.int32), torch.cat([rows_cross, rows_wait])


def ragged_plan(pos, bucket, rec_of, len, M, S, k):
    """mhppo_ragged_plan (CUDA): ragged_plan_torch's three results, queued on the current stream."""
    NS = M * S
    dev = pos.device
    L = _lib.lib()
    row0 = torch.empty(NS, dtype=torch.int64, device=dev)
    len_rec = torch.empty(NS, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    work = torch.empty(max(1, int(L.mhppo_ragged_work_bytes(NS)) // 8), dtype=torch.int64, device=dev)
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(L.mhppo_ragged_plan(p(pos), p(bucket), p(rec_of), p(len), M, S, int(k), p(row0), p(len_rec), p(info),
                                       p(work), _lib.stream_ptr(device=dev)))
    return row0, len_rec, info


def _boot_args(pos, bucket, rec_of, len, trunc, M, S, k, obs_tm, feat_tail, n_in, who):
    """The checked, contiguous operands of boot_values / boot_values_torch."""
    NS, k = M * S, int(k)
    dev = pos.device
    if k < 1:
        raise ValueError(f"{who}: k < 1")
    for name, x, dt, n in (("pos", pos, torch.int64, NS), ("bucket", bucket, torch.int8, NS),
                           ("len", len, torch.int32, M), ("trunc", trunc, torch.uint8, M)):
        if not torch.is_tensor(x) or x.dtype != dt or x.numel() != n or x.device != dev:
            raise ValueError(f"{who}: {name} is a {dt} [{n}] tensor on the records' device")
    if rec_of is not None and (rec_of.dtype != torch.int32 or rec_of.numel() < NS or rec_of.device != dev):
        raise ValueError(f"{who}: rec_of is an int32 [{NS}] tensor on the records' device, or None")
    if (obs_tm.dtype != torch.float32 or obs_tm.device != dev or obs_tm.shape[-1] != n_in
            or obs_tm.numel() % max(1, NS * n_in) or (NS and obs_tm.numel() // (NS * n_in) < k)):
        raise ValueError(f"{who}: obs_tm is a float32 [>= {k}, {NS}, {n_in}] tensor on the records' device")
    if feat_tail is not None and (feat_tail.dtype != torch.float32 or feat_tail.device != dev
                                  or feat_tail.numel() != NS * n_in):
        raise ValueError(f"{who}: feat_tail is a float32 [{M}, {S}, {n_in}] tensor on the records' device, or None")
    c = lambda x: None if x is None else x.contiguous()
    return (c(pos.reshape(NS)), c(bucket.reshape(NS)), None if rec_of is None else c(rec_of.reshape(-1)[:NS]),
            c(len.reshape(M)), c(trunc.reshape(M)), c(obs_tm.reshape(-1 if NS else 0, NS, n_in)),
            None if feat_tail is None else c(feat_tail.reshape(NS, n_in)))


def boot_values_torch(critic0, critic1, pos, bucket, rec_of, len, trunc, M, S, k, cut_truncates, obs_tm, feat_tail=None):
    """mhppo_boot_values in torch ops (any device): its executable specification and the CPU path.
    Per segment s = r S + i: col = rec_of[s] (s with rec_of None; nothing for col < 0); the stream ended
    iff 1 <= len[r] <= k, with L = len[r] and the truncation flag trunc[r]; else it was cut at L = k,
    a truncation iff cut_truncates.  A truncated segment of a used column (pos[col] >= 0) gets
    v_boot[col] = critic(row), critic1 for bucket[col] != 0 else critic0, row = obs_tm[L, col] for
    L < k and feat_tail[s] for L == k (None: no bootstrap there); every other column 0.  V comes from
    _critic_values: mhppo_mlp_forward on the GPU.  Rows the rule does not select are replaced by zeros
    before the forward.  -> float32 [M S]; nothing is read back."""
    n_in = critic0.n_in
    if critic1.n_in != n_in:
        raise ValueError("boot_values_torch: the critics differ in n_in")
    pos, bucket, rec_of, ln, trunc, obs, tail = _boot_args(pos, bucket, rec_of, len, trunc, M, S, k, obs_tm, feat_tail,
                                                           n_in, "boot_values_torch")
    NS, k = M * S, int(k)
    dev = pos.device
    s = torch.arange(NS, device=dev)
    r = torch.div(s, S, rounding_mode="floor")
    col = s if rec_of is None else rec_of.long()
    has = col >= 0
    colc = col.clamp_min(0)
    lr = ln.long().index_select(0, r)
    ended = (lr >= 1) & (lr <= k)
    L = torch.where(ended, lr, torch.full_like(lr, k))
    tr = torch.where(ended, trunc.index_select(0, r) != 0, torch.full_like(ended, bool(cut_truncates)))
    rec = L < k
    sel = has & (pos.index_select(0, colc) >= 0) & tr & (rec | (tail is not None))
    b1 = bucket.index_select(0, colc) != 0
    rows = obs[torch.where(rec, L, torch.zeros_like(L)), colc]
    if tail is not None:
        rows = torch.where(rec[:, None], rows, tail)
    rows = torch.where(sel[:, None], rows, torch.zeros((), dtype=torch.float32, device=dev))
    v0, v1 = _critic_values(critic0, rows).float(), _critic_values(critic1, rows).float()
    v = torch.where(sel, torch.where(b1, v1, v0), torch.zeros((), dtype=torch.float32, device=dev))
    out = torch.zeros(NS + 1, dtype=torch.float32, device=dev)
    return out.scatter_(0, torch.where(has, col, torch.full_like(col, NS)), v)[:NS]


def boot_values(critic0, critic1, pos, bucket, rec_of, len, trunc, M, S, k, cut_truncates, obs_tm, feat_tail=None):
    """mhppo_boot_values (CUDA): boot_values_torch's result in one launch on the current stream, V bit
    for bit forward_rows'."""
    n_in = critic0.n_in
    pos, bucket, rec_of, ln, trunc, obs, tail = _boot_args(pos, bucket, rec_of, len, trunc, M, S, k, obs_tm, feat_tail,
                                                           n_in, "boot_values")
    dev = pos.device
    d0, keep0 = critic0.mlp_desc()
    d1, keep1 = critic1.mlp_desc()
    if dev.type != "cuda" or keep0.device != dev or keep1.device != dev:
        raise ValueError("boot_values: the critics must live on the records' GPU")
    v_boot = torch.zeros(M * S, dtype=torch.float32, device=dev)
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mhppo_boot_values(ctypes.byref(d0), ctypes.byref(d1), p(pos), p(bucket), p(rec_of), p(ln),
                                                p(trunc), M, S, int(k), int(bool(cut_truncates)), p(obs), p(tail),
                                                p(v_boot), _lib.stream_ptr(device=dev)))
    return v_boot


def _batch_boot(batch, boot, plan_pos, plan_bucket, rec_of, ln, k, native):
    """v_boot of a ragged batch under boot = (critic_cross, critic_wait), or None: no boot, or a batch
    without the truncation flags (ExternalRollout without bootstrap)."""
    trunc = getattr(batch, "trunc", None)
    if boot is None or trunc is None:
        return None
    f = boot_values if native else boot_values_torch
    return f(boot[0], boot[1], plan_pos, plan_bucket, rec_of, ln, trunc, batch.N, batch.S, k,
             getattr(batch, "cut_truncates", True), batch.obs_c_tm, getattr(batch, "feat_tail", None))


def _ragged_views(both, rows_cross, rows_wait, n_cross, n_wait):
    w0 = (rows_cross + 3) // 4 * 4
    keys = ("obs", "act", "logp", "ret", "rew")
    cross_r = {k: both[k][:rows_cross] for k in keys}
    wait_r = {k: both[k][w0:w0 + rows_wait] for k in keys}
    cross_r["n_seg"], wait_r["n_seg"] = n_cross, n_wait
    cross_r["rows"], wait_r["rows"] = rows_cross, rows_wait
    return cross_r, wait_r


def bucket_segments_ragged_native(batch, fix_bucket=False, status=None, gae=None, boot=None):
    """bucket_segments on the GPU for a batch with early episode ends (batch.len int32 [N], batch.steps
    = k recorded steps; ExternalRollout(early_end=True)): mhppo_bucket_plan, then mhppo_ragged_plan
    (every segment's first row and length), the reward-to-go or GAE scan cut at the lengths, and ONE
    ragged scatter of both buckets into the shared buffer that also folds the cross / wait reward
    sums.  A segment of a stream of length L owns L contiguous rows; the cross rows start at row 0, the
    wait rows at W0 = rows_cross rounded up to a multiple of 4.  The one host read -- the plan's sizes
    and status word and the two row counts -- comes before the scatter is queued.  The returned dicts
    have bucket_segments' keys and `rows`; the choice batch is unchanged (its ret is the ep_min frozen
    at each stream's end).  boot = (critic_cross, critic_wait) on a batch with trunc: mhppo_boot_values is
    queued after the ragged plan and the scan that runs starts every truncated segment from its v_boot
    (mhppo_returns_scan_tm_boot / mhppo_gae_tm_boot); the host read stays the only one."""
    N, S, P, T = batch.N, batch.S, batch.P, batch.T
    NS = N * S
    dev = batch.a_d.device
    L = _lib.lib()
    ln, k = _ragged_steps(batch)
    plan = bucket_plan(batch, fix_bucket, status)
    rec_of = getattr(batch, "rec_of", None)
    rec_of = None if rec_of is None else rec_of.contiguous()
    row0, len_rec, rinfo = ragged_plan(plan["pos"], plan["bucket"], rec_of, ln, N, S, k)
    v_boot = _batch_boot(batch, boot, plan["pos"], plan["bucket"], rec_of, ln, k, native=True)
    if gae is None:
        ret_tm = returns_scan_tm(batch.rew_tm, len_rec=len_rec, v_boot=v_boot)
    else:
        critic_cross, critic_wait, gamma, lam = gae
        ret_tm = gae_targets_tm(batch.obs_c_tm, batch.rew_tm, critic_cross, critic_wait, plan["pos"], plan["bucket"],
                                gamma, lam, len_rec=len_rec, v_boot=v_boot)
    info = plan["info"]
    n = NS * T + 3
    both = dict(obs=torch.empty(n, NF_C, dtype=torch.float32, device=dev),
                act=torch.empty(n, dtype=torch.float32, device=dev),
                logp=torch.empty(n, dtype=torch.float32, device=dev),
                ret=torch.empty(n, dtype=torch.float32, device=dev),
                rew=torch.empty(n, dtype=torch.float64, device=dev))
    one = _lib.BucketDst(*[both[k_].data_ptr() for k_ in ("obs", "act", "logp", "ret", "rew")])
    dst = (_lib.BucketDst * 2)(one, one)  # cross and wait rows share the buffer (bucket[] keys the sums)
    srcs = [x.contiguous() for x in (batch.obs_c_tm, batch.act_tm, batch.logp_tm)]
    rew_tm = batch.rew_tm.contiguous()
    p = _lib.ptr
    args = (p(row0), p(plan["bucket"]), p(len_rec), NS, T, *[p(x) for x in srcs], p(ret_tm), p(rew_tm), dst,
            ctypes.c_void_p(info.data_ptr() + 48), p(plan["work"]), _lib.stream_ptr(device=dev))
    n_cross, n_wait, n_all, st, rows_cross, rows_wait = torch.cat([info[:4], rinfo]).tolist()  # the one host read
    if status is not None:
        if st:
            status.zero_()
        raise_if_nan_status(st)
    with torch.cuda.device(dev):
        _lib.check(L.mhppo_bucket_scatter_ragged(*args))
    cross_r, wait_r = _ragged_views(both, rows_cross, rows_wait, n_cross, n_wait)
    choice = {k_: plan[k_][:n_all] for k_ in ("obs", "act", "logp", "ret")}
    choice["n_seg"] = n_all
    f64 = info[4:9].view(torch.float64)
    choice["counts"] = f64[0:2]
    choice["rew_sums"] = f64[2:5]
    return cross_r, wait_r, choice


def _tree_torch(v, NT):
    """block_prims.h's halving tree over NT threads: [..., NT] -> [...]"""
    v = v.clone()
    s = NT // 2
    while s:
        v[..., :s] = v[..., :s] + v[..., s:2 * s]
        s //= 2
    return v[..., 0]


def _fold_torch(x, NT, CHAINS):
    """block_prims.h's fold (k_fold<NT, CHAINS>, or strided_sum + block_sum) of float64 [..., n] in
    torch ops: element b + u NT + j CHAINS NT goes to chain u of thread b in ascending j, four chains
    combine as (a0 + a1) + (a2 + a3), then the tree.  Equal order, equal bits."""
    n, step = x.shape[-1], CHAINS * NT
    rounds = max(1, -(-n // step))
    pad = torch.zeros(x.shape[:-1] + (rounds * step,), dtype=torch.float64, device=x.device)
    pad[..., :n] = x
    pad = pad.reshape(x.shape[:-1] + (rounds, CHAINS, NT))
    acc = torch.zeros(x.shape[:-1] + (CHAINS, NT), dtype=torch.float64, device=x.device)
    for r in range(rounds):
        acc = acc + pad[..., r, :, :]
    a = acc[..., 0, :] if CHAINS == 1 else (acc[..., 0, :] + acc[..., 1, :]) + (acc[..., 2, :] + acc[..., 3, :])
    return _tree_torch(a, NT)


def scatter_sums_torch(rew_tm, own, bucket):
    """The two reward sums of mhppo_bucket_scatter_sums / _scatter_ragged onto zeroed rew_sums, in
    their order (csrc/ppo_batch.hip k_bucket_scatter at its 1024-thread block): rew_tm float64 [T, NS],
    own bool [T, NS] (the record is scattered), bucket int8 [NS].  A block is 64 segments x 16 steps;
    each step's wave adds its 64 records by the xor butterfly, the block its 16 waves in index order;
    the partials (block y gridDim.x + x) are folded by k_fold<1024, 4>.  -> float64 [2]"""
    return _scatter_sums_sel(rew_tm, [own & ((bucket != 0) == bool(k))[None, :] for k in range(2)])


def _scatter_sums_sel(rew_tm, sels):
    """scatter_sums_torch with each bucket's records given as a bool [T, NS] mask (the lanes scatter: a
    column's bucket can change from one episode to the next)."""
    T, NS = rew_tm.shape
    dev = rew_tm.device
    gx, gy = -(-NS // 64), -(-T // 16)
    lanes = torch.arange(64, device=dev)
    out = []
    for sel in sels:
        r = torch.zeros((gy * 16, gx * 64), dtype=torch.float64, device=dev)
        r[:T, :NS] = torch.where(sel, 0.0 + rew_tm.float().double(), torch.zeros((), dtype=torch.float64, device=dev))
        v = r.reshape(gy, 16, gx, 64)
        for m in (32, 16, 8, 4, 2, 1):
            v = v + v[..., lanes ^ m]
        a = torch.zeros((gy, gx), dtype=torch.float64, device=dev)
        for q in range(16):
            a = a + v[:, q, :, 0]
        out.append(0.0 + _fold_torch(a.reshape(gy * gx), 1024, 4))
    return torch.stack(out)


def plan_ep_sum_torch(ep_min, exist):
    """mhppo_bucket_plan's rew_sums[2] in its order: (double)(float)ep_min of the existing segments
    through the 256-thread tree per block of 256 segments, the block partials folded by 256 threads
    with one chain.  -> float64 scalar"""
    e = torch.where(exist.reshape(-1), ep_min.reshape(-1).float().double(), 0.0)
    nb = max(1, -(-e.numel() // 256))
    pad = torch.zeros(nb * 256, dtype=torch.float64, device=e.device)
    pad[:e.numel()] = e
    return _fold_torch(_tree_torch(pad.reshape(nb, 256), 256), 256, 1)


def _critic_values(critic, obs):
    """V of observation rows for the torch paths: the native forward on the GPU (the bits the GAE
    kernel uses), torch's forward on the CPU."""
    with torch.no_grad():
        if obs.device.type == "cuda":
            return critic.forward_rows(obs.contiguous())
        return critic(obs).reshape(-1)


def bucket_segments_ragged_torch(batch, fix_bucket=False, status=None, plan_out=None, gae=None, boot=None):
    """bucket_segments_ragged_native in torch ops (any device): its specification and the CPU path.
    Everything is queued before the one host read.  plan_out: a dict that receives pos, bucket, row0
    and len_rec (and v_boot, when there is one; tests).  With gae, V comes from _critic_values on the
    time-major records; with boot on a batch with trunc, v_boot from boot_values_torch."""
    N, S, P, T = batch.N, batch.S, batch.P, batch.T
    NS = N * S
    ln, k = _ragged_steps(batch)
    exist, cross, wait = _segment_masks(batch, fix_bucket)
    dev = exist.device
    cc, cw = torch.cumsum(cross, 0), torch.cumsum(wait, 0)
    n_cross_d = cc[-1] if NS else torch.zeros((), dtype=torch.int64, device=dev)
    w0s = torch.div(n_cross_d + 3, 4, rounding_mode="floor") * 4
    pos = torch.where(cross, cc - 1, torch.where(wait, w0s + cw - 1, -1))
    bucket = wait.to(torch.int8)
    rec_of = getattr(batch, "rec_of", None)
    if rec_of is not None:  # the compact layout: positions and buckets are per record
        idx = torch.where(rec_of[:NS] >= 0, rec_of[:NS], NS).long()
        pos = torch.full((NS + 1,), -1, dtype=pos.dtype, device=dev).scatter_(0, idx, pos)[:NS]
        bucket = torch.zeros(NS + 1, dtype=torch.int8, device=dev).scatter_(0, idx, bucket)[:NS]
    row0, len_rec, rinfo = ragged_plan_torch(pos, bucket, rec_of, ln, N, S, k)
    v_boot = _batch_boot(batch, boot, pos, bucket, rec_of, ln, k, native=False)
    if plan_out is not None:
        plan_out.update(pos=pos, bucket=bucket, row0=row0, len_rec=len_rec)
        if v_boot is not None:
            plan_out.update(v_boot=v_boot)
    rew_tm = batch.rew_tm.reshape(T, NS)
    obs_tm = batch.obs_c_tm.reshape(T, NS, NF_C)
    if gae is None:
        ret_tm = returns_scan_tm(rew_tm, len_rec=len_rec, v_boot=v_boot)
    else:
        v0, v1 = (_critic_values(c, obs_tm.reshape(T * NS, NF_C)).reshape(T, NS) for c in gae[:2])
        used_len = torch.where(pos >= 0, len_rec, torch.zeros_like(len_rec))
        ret_tm = gae_targets_torch(rew_tm, torch.where((bucket != 0)[None, :], v1, v0), gae[2], gae[3], len_rec=used_len,
                                   v_boot=v_boot)
    # record (t, b) with row0[b] >= 0 and t < len_rec[b] goes to row row0[b] + t; every other record to
    # a spare row past the buffer's end
    n = NS * T + 3
    tt = torch.arange(T, device=dev)[:, None]
    own = (row0 >= 0)[None, :] & (tt < len_rec[None, :])
    rows = torch.where(own, row0[None, :] + tt, n).reshape(-1)
    both = {}
    for key, x, dt in (("obs", obs_tm, torch.float32), ("act", batch.act_tm, torch.float32),
                       ("logp", batch.logp_tm, torch.float32), ("ret", ret_tm, torch.float32),
                       ("rew", rew_tm, torch.float64)):
        x = x.reshape(T * NS, -1)
        buf = torch.zeros((n + 1, x.shape[1]), dtype=dt, device=dev)
        buf[rows] = x
        both[key] = buf[:n] if key == "obs" else buf[:n, 0]
    # the reward sums, in the fixed orders of mhppo_bucket_scatter_ragged and mhppo_bucket_plan
    choice, counts = _choice_torch(batch, exist)
    rew_sums = torch.cat([scatter_sums_torch(rew_tm, own, bucket), plan_ep_sum_torch(batch.ep_min, exist).reshape(1)])
    sizes = [n_cross_d, cw[-1] if NS else n_cross_d, exist.sum(), rinfo[0], rinfo[1]]
    if status is not None:
        sizes.append(status.reshape(-1)[0].to(torch.int64))
    sizes = torch.stack(sizes).tolist()  # the one host read
    if status is not None:
        if sizes[5]:
            status.zero_()
        raise_if_nan_status(sizes[5])
    n_cross, n_wait, n_all, rows_cross, rows_wait = sizes[:5]
    cross_r, wait_r = _ragged_views(both, rows_cross, rows_wait, n_cross, n_wait)
    choice = {k_: v[:n_all] for k_, v in choice.items()}
    choice["n_seg"] = n_all
    choice["counts"] = counts
    choice["rew_sums"] = rew_sums
    return cross_r, wait_r, choice


# ------------------------------------------------------------------ auto-reset lanes
def _lanes_fields(batch):
    """(E, M, S, T, k, t0, len, cut, plan view) of a batch with auto-reset lanes, checked.  The plan view
    is the batch as mhppo_bucket_plan and the torch bucket rule take it: one "env" per lane, N = E M."""
    E, M, S, T = int(batch.lanes), int(batch.M), batch.S, batch.T
    k = int(getattr(batch, "steps", T))
    dev = batch.a_d.device
    if E < 1 or not 1 <= k <= T:
        raise ValueError(f"a lanes batch has lanes >= 1 and 1 <= steps <= T = {T}, not {E}, {k}")
    out = []
    for name, dt in (("t0", torch.int32), ("len", torch.int32), ("cut", torch.uint8)):
        x = getattr(batch, name, None)
        if not torch.is_tensor(x) or x.dtype != dt or x.numel() != E * M or x.device != dev:
            raise ValueError(f"a lanes batch's {name} is a {dt} [{E * M}] tensor on the batch's device")
        out.append(x.reshape(E * M).contiguous())
    view = RolloutBatch(N=E * M, S=S, P=batch.P, T=T, a_d=batch.a_d, closest=batch.closest, exist=batch.exist,
                        ep_min=batch.ep_min, feat_d=batch.feat_d, logp_d=batch.logp_d, rec_of=None)
    return (E, M, S, T, k, *out, view)


def _lane_columns(E, M, S, dev):
    """per lane-segment q = v S + i, v = e M + r: (v, the record column r S + i)"""
    q = torch.arange(E * M * S, device=dev)
    v = torch.div(q, S, rounding_mode="floor")
    return v, (v % M) * S + q % S


def returns_scan_tm_lanes_torch(rew_tm, M, S, E, gamma, pos, t0, len, cut, v_boot=None):
    """mhppo_returns_scan_tm_lanes in torch ops (any device): rew_tm float64 [T, M S] -> float32 [T, M S].
    Lane-segment q = v S + i with pos[q] >= 0 scans column r S + i over t = t0[v] + L - 1 .. t0[v] in float64,
    L = len[v], from G = float64(v_boot[col]) where cut[v] and v_boot is given, else 0; every record in no
    used lane is 0."""
    T = rew_tm.shape[0]
    NS = M * S
    rew = rew_tm.reshape(T, NS)
    dev = rew.device
    v, col = _lane_columns(E, M, S, dev)
    used = pos.reshape(-1) >= 0
    T0 = t0.long()[v].clamp(0, T)
    L = torch.minimum(len.long()[v].clamp_min(0), T - T0)
    g = torch.zeros(v.numel(), dtype=torch.float64, device=dev)
    if v_boot is not None:
        g = torch.where(used & (cut[v] != 0) & (L > 0), v_boot.reshape(NS)[col].double(), g)
    ret = torch.zeros((T, NS), dtype=torch.float32, device=dev)
    for j in range(T - 1, -1, -1):  # the lane's own step j, wall-clock t0 + j
        on = used & (j < L)
        tt = (T0 + j).clamp_max(T - 1)
        g = torch.where(on, rew[tt, col] + gamma * g, g)
        ret[tt[on], col[on]] = g[on].float()
    return ret.reshape(rew_tm.shape)


def returns_scan_tm_lanes(rew_tm, M, S, E, gamma, pos, t0, len, cut, v_boot=None):
    """mhppo_returns_scan_tm_lanes (CUDA): returns_scan_tm_lanes_torch's result, a memset and one launch
    on the current stream."""
    T = rew_tm.shape[0]
    r = rew_tm.reshape(T, M * S).contiguous()
    out = torch.empty(r.shape, dtype=torch.float32, device=r.device)
    if v_boot is not None:
        v_boot = _check_v_boot(v_boot, M * S, r.device, "returns_scan_tm_lanes")
    p = _lib.ptr
    with torch.cuda.device(r.device):
        _lib.check(_lib.lib().mhppo_returns_scan_tm_lanes(p(r), p(out), M, S, E, T, gamma, p(pos), p(t0), p(len), p(cut),
                                                          p(v_boot), _lib.stream_ptr(device=r.device)))
    return out.reshape(rew_tm.shape)


def _lanes_boot(batch, boot, pos, bucket, E, M, S, k, cut, native):
    """v_boot float32 [M S] per record column of a lanes batch under boot = (critic_cross, critic_wait), or
    None without boot: mhppo_boot_values over the M streams, each with the pos / bucket of its open lane
    (the one cut when the batch was taken; -1 where the stream has none), len = 0 -- every stream then
    counts as cut at k -- and the batch's cut_truncates and feat_tail."""
    if boot is None:
        return None
    dev = pos.device
    c = cut.reshape(E, M)
    v_open = c.to(torch.int64).argmax(0) * M + torch.arange(M, device=dev)  # at most one lane of a stream is open
    q = v_open[:, None] * S + torch.arange(S, device=dev)[None, :]
    pos_open = torch.where((c != 0).any(0)[:, None], pos[q], torch.full_like(q, -1)).reshape(M * S)
    f = boot_values if native else boot_values_torch
    return f(boot[0], boot[1], pos_open, bucket[q].reshape(M * S).contiguous(), None,
             torch.zeros(M, dtype=torch.int32, device=dev), torch.zeros(M, dtype=torch.uint8, device=dev), M, S, k,
             getattr(batch, "cut_truncates", True), batch.obs_c_tm, getattr(batch, "feat_tail", None))


def _lanes_no_gae(gae):
    if gae is not None:
        raise ValueError("bucket_segments: gae (gae_lambda) with auto-reset lanes is out of scope: the "
                         "lambda-return kernel takes one length per column")


def bucket_segments_lanes_native(batch, fix_bucket=False, status=None, gae=None, boot=None):
    """bucket_segments on the GPU for a batch with auto-reset lanes (ExternalRollout(auto_reset=E)):
    mhppo_bucket_plan and mhppo_ragged_plan over the N = E M lanes with the lanes' len (a lane never
    started has exist = 0, hence pos < 0 and no row), mhppo_boot_values for the lanes cut at the window's
    end (boot), mhppo_returns_scan_tm_lanes over the wall-clock records, and ONE scatter of both buckets
    into the shared buffer that also folds the cross / wait reward sums (mhppo_bucket_scatter_lanes).
    Cross rows start at row 0, wait rows at W0 = rows_cross rounded up to a multiple of 4; segments follow
    the lane-segment order (lane e, stream r, slot i), a lane-segment of length L owns L contiguous rows;
    the choice batch has one row per existing lane-segment in that order, ret = (float)ep_min of the lane.
    The dicts' keys are the ragged path's; the one host read comes before the scatter is queued."""
    _lanes_no_gae(gae)
    E, M, S, T, k, t0, ln, cut, view = _lanes_fields(batch)
    NS = M * S
    dev = batch.a_d.device
    L = _lib.lib()
    plan = bucket_plan(view, fix_bucket, status)
    row0, _, rinfo = ragged_plan(plan["pos"], plan["bucket"], None, ln, E * M, S, k)
    v_boot = _lanes_boot(batch, boot, plan["pos"], plan["bucket"], E, M, S, k, cut, native=True)
    ret_tm = returns_scan_tm_lanes(batch.rew_tm, M, S, E, GAMMA, plan["pos"], t0, ln, cut, v_boot)
    info = plan["info"]
    n = NS * T + 3  # a stream's lanes do not overlap: at most k rows per column
    both = dict(obs=torch.empty(n, NF_C, dtype=torch.float32, device=dev),
                act=torch.empty(n, dtype=torch.float32, device=dev),
                logp=torch.empty(n, dtype=torch.float32, device=dev),
                ret=torch.empty(n, dtype=torch.float32, device=dev),
                rew=torch.empty(n, dtype=torch.float64, device=dev))
    one = _lib.BucketDst(*[both[k_].data_ptr() for k_ in ("obs", "act", "logp", "ret", "rew")])
    dst = (_lib.BucketDst * 2)(one, one)  # cross and wait rows share the buffer (bucket[] keys the sums)
    srcs = [x.contiguous() for x in (batch.obs_c_tm, batch.act_tm, batch.logp_tm)]
    rew_tm = batch.rew_tm.contiguous()
    p = _lib.ptr
    args = (p(row0), p(plan["bucket"]), p(t0), p(ln), M, S, E, T, *[p(x) for x in srcs], p(ret_tm), p(rew_tm), dst,
            ctypes.c_void_p(info.data_ptr() + 48), p(plan["work"]), _lib.stream_ptr(device=dev))
    n_cross, n_wait, n_all, st, rows_cross, rows_wait = torch.cat([info[:4], rinfo]).tolist()  # the one host read
    if status is not None:
        if st:
            status.zero_()
        raise_if_nan_status(st)
    with torch.cuda.device(dev):
        _lib.check(L.mhppo_bucket_scatter_lanes(*args))
    cross_r, wait_r = _ragged_views(both, rows_cross, rows_wait, n_cross, n_wait)
    choice = {k_: plan[k_][:n_all] for k_ in ("obs", "act", "logp", "ret")}
    choice["n_seg"] = n_all
    f64 = info[4:9].view(torch.float64)
    choice["counts"] = f64[0:2]
    choice["rew_sums"] = f64[2:5]
    return cross_r, wait_r, choice


def bucket_segments_lanes_torch(batch, fix_bucket=False, status=None, plan_out=None, gae=None, boot=None):
    """bucket_segments_lanes_native in torch ops (any device): its specification and the CPU path.
    Everything is queued before the one host read.  plan_out: a dict that receives pos, bucket, row0, ret_tm
    and v_boot (tests)."""
    _lanes_no_gae(gae)
    E, M, S, T, k, t0, ln, cut, view = _lanes_fields(batch)
    NS, NL = M * S, E * M * S
    exist, cross, wait = _segment_masks(view, fix_bucket)
    dev = exist.device
    cc, cw = torch.cumsum(cross, 0), torch.cumsum(wait, 0)
    n_cross_d = cc[-1] if NL else torch.zeros((), dtype=torch.int64, device=dev)
    w0s = torch.div(n_cross_d + 3, 4, rounding_mode="floor") * 4
    pos = torch.where(cross, cc - 1, torch.where(wait, w0s + cw - 1, -1))
    bucket = wait.to(torch.int8)
    row0, _, rinfo = ragged_plan_torch(pos, bucket, None, ln, E * M, S, k)
    v_boot = _lanes_boot(batch, boot, pos, bucket, E, M, S, k, cut, native=False)
    rew_tm = batch.rew_tm.reshape(T, NS)
    obs_tm = batch.obs_c_tm.reshape(T, NS, NF_C)
    ret_tm = returns_scan_tm_lanes_torch(rew_tm, M, S, E, GAMMA, pos, t0, ln, cut, v_boot)
    if plan_out is not None:
        plan_out.update(pos=pos, bucket=bucket, row0=row0, ret_tm=ret_tm, v_boot=v_boot)
    # record (t0 + j, col) of a used lane-segment goes to row row0 + j, j < len; every other pair (j, q) to
    # a spare row past the buffer's end
    n = NS * T + 3
    v, col = _lane_columns(E, M, S, dev)
    jj = torch.arange(T, device=dev)[:, None]
    own = (row0 >= 0)[None, :] & (jj < ln.long()[v][None, :])  # [T, NL]
    rows = torch.where(own, row0[None, :] + jj, n).reshape(-1)
    rec = torch.where(own, (t0.long()[v][None, :] + jj) * NS + col[None, :], 0).reshape(-1)
    both = {}
    for key, x, dt in (("obs", obs_tm, torch.float32), ("act", batch.act_tm, torch.float32),
                       ("logp", batch.logp_tm, torch.float32), ("ret", ret_tm, torch.float32),
                       ("rew", rew_tm, torch.float64)):
        x = x.reshape(T * NS, -1)
        buf = torch.zeros((n + 1, x.shape[1]), dtype=dt, device=dev)
        buf[rows] = x[rec]
        both[key] = buf[:n] if key == "obs" else buf[:n, 0]
    # the reward sums, in the fixed orders of mhppo_bucket_scatter_lanes and mhppo_bucket_plan
    sels = []
    for b in range(2):
        m = torch.zeros(T * NS + 1, dtype=torch.bool, device=dev)
        m[torch.where(own & ((bucket != 0) == bool(b))[None, :], rec.reshape(T, NL), T * NS).reshape(-1)] = True
        sels.append(m[:T * NS].reshape(T, NS))
    choice, counts = _choice_torch(view, exist)
    rew_sums = torch.cat([_scatter_sums_sel(rew_tm, sels), plan_ep_sum_torch(batch.ep_min, exist).reshape(1)])
    sizes = [n_cross_d, cw[-1] if NL else n_cross_d, exist.sum(), rinfo[0], rinfo[1]]
    if status is not None:
        sizes.append(status.reshape(-1)[0].to(torch.int64))
    sizes = torch.stack(sizes).tolist()  # the one host read
    if status is not None:
        if sizes[5]:
            status.zero_()
        raise_if_nan_status(sizes[5])
    n_cross, n_wait, n_all, rows_cross, rows_wait = sizes[:5]
    cross_r, wait_r = _ragged_views(both, rows_cross, rows_wait, n_cross, n_wait)
    choice = {k_: x[:n_all] for k_, x in choice.items()}
    choice["n_seg"] = n_all
    choice["counts"] = counts
    choice["rew_sums"] = rew_sums
    return cross_r, wait_r, choice


def scatter_buckets(seg0, seg1, NS, T, obs_tm, act_tm, logp_tm, ret_tm, rew_tm):
    """Two segment-major buckets of time-major records (mhppo_bucket_scatter): row
    (k, t) = k*T + t of bucket b is record t*NS + seg_b[k] (segments disjoint)."""
    dev = obs_tm.device
    pos = torch.full((NS,), -1, dtype=torch.int64, device=dev)
    bucket = torch.zeros(NS, dtype=torch.int8, device=dev)
    for b, seg in enumerate((seg0, seg1)):
        pos[seg] = torch.arange(int(seg.numel()), dtype=torch.int64, device=dev)
        bucket[seg] = b
    return scatter_positions(pos, bucket, (int(seg0.numel()), int(seg1.numel())), NS, T, obs_tm, act_tm, logp_tm,
                             ret_tm, rew_tm)


def scatter_positions(pos, bucket, sizes, NS, T, obs_tm, act_tm, logp_tm, ret_tm, rew_tm):
    """scatter_buckets with the segments given as positions: segment s goes to row block pos[s]
    of bucket bucket[s] (pos < 0: no bucket); sizes = the two buckets' segment counts."""
    dev = obs_tm.device
    if dev.type != "cuda":  # the torch path's CPU form: the same rows by index ops
        outs = []
        seg_all = torch.nonzero(pos >= 0).squeeze(1)
        for b, n in enumerate(sizes):
            seg = seg_all[bucket[seg_all] == b]
            rows = (pos[seg].long()[:, None] * T + torch.arange(T)[None, :]).reshape(-1)
            o = {}
            for k, x, dt in (("obs", obs_tm, torch.float32), ("act", act_tm, torch.float32),
                             ("logp", logp_tm, torch.float32), ("ret", ret_tm, torch.float32),
                             ("rew", rew_tm, torch.float64)):
                x = x.reshape(T, NS, -1)
                buf = torch.zeros((n * T, x.shape[2]), dtype=dt)
                buf[rows] = x[:, seg].transpose(0, 1).reshape(-1, x.shape[2])
                o[k] = buf if k == "obs" else buf[:, 0]
            o["n_seg"] = n
            outs.append(o)
        return outs
    outs, dst = [], (_lib.BucketDst * 2)()  # one size: bucket 1 unused (every bucket[s] = 0)
    for b, n in enumerate(sizes):
        o = dict(obs=torch.empty(n * T, NF_C, dtype=torch.float32, device=dev),
                 act=torch.empty(n * T, dtype=torch.float32, device=dev),
                 logp=torch.empty(n * T, dtype=torch.float32, device=dev),
                 ret=torch.empty(n * T, dtype=torch.float32, device=dev),
                 rew=torch.empty(n * T, dtype=torch.float64, device=dev), n_seg=n)
        dst[b] = _lib.BucketDst(*[o[k].data_ptr() for k in ("obs", "act", "logp", "ret", "rew")])
        outs.append(o)
    srcs = [x.contiguous() for x in (obs_tm, act_tm, logp_tm, ret_tm, rew_tm)]
    _lib.check(_lib.lib().mhppo_bucket_scatter(_lib.ptr(pos), _lib.ptr(bucket), NS, T, *[_lib.ptr(x) for x in srcs],
                                               dst, _lib.stream_ptr(device=dev)))
    return outs
