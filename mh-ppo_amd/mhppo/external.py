"""External rollouts: one PPO iteration's batch from any simulator's observation rows.

`ExternalRollout` is RolloutGPU.collect with the env taken out: the training policy's draws come
from a SamplingSession (mhppo.policy) on the rows the simulator hands over, the simulator steps on
the actions it gets back, and the collector's bookkeeping between a sampling step and the bucketing
-- the time-major records, the compact record layout of the scalable variant (rec_of), the float64
reward record and the NaN-propagating episodic minimum of reward_light -- is the native record pass
(mhppo_record_begin / mhppo_record_step, include/mhppo.h, csrc/rollout_record.hip).  The RolloutBatch
it returns has the fields RolloutGPU.collect returns and goes to bucket_segments unchanged; driven by
a VecCrosswalk it is the collector's batch bit for bit.

By default episodes have the fixed length T, as in the collector and the reference's drivers: the time
limit is terminal and nothing else is, and a simulator's `done` is ignored.  ExternalRollout(early_end=
True) takes the per-stream `done` a vectorised simulator returns: the step that first reports it is the
stream's last, terminal exactly as the time limit is (V = 0 after it, no bootstrap), and nothing of the
later steps reaches a bucket row, a return, ep_min or a reward sum (mhppo_record_step_done and the ragged
bucketing, mhppo.rollout.bucket_segments_ragged_native).

ExternalRollout(early_end=True, bootstrap=True) tells a truncation from an end (Gymnasium's terminated /
truncated pair, a T-step window cut out of a longer scene): record takes a second per-stream flag,
`truncated`, read at the step that first reports done, and a stream still running when the batch is
taken is cut at k steps, which is a truncation iff cut_truncates (the default).  The targets of a
truncated segment of length L start from V(s_L) under its bucket's critic instead of 0
(bucket_segments(boot=...), mhppo_boot_values); s_L is record L of the segment for L < k and a row of
finish(obs) for L == k.

ExternalRollout(auto_reset=E) is for simulators that reset a stream the moment it reports done (Gymnasium
vector envs, SB3's VecEnv, batched sims): a stream plays episode after episode inside the T-step window,
up to E of them -- its LANES, lane e M + r being the e-th episode of stream r.  Every episode has its own
choice decision, drawn from its first row, its own bucket, episodic minimum and targets; the episode
running when the batch is taken is cut there (mhppo_lanes_*, csrc/rollout_lanes.hip, and the lanes
bucketing, mhppo.rollout.bucket_segments_lanes_native).  Out of scope, each a ValueError: gae_lambda with
auto_reset (the lambda-return kernel takes one length per column), a mid-window truncated flag (it needs
the simulator's final observation), next-step auto-reset simulators (the row after a done must already be
the new episode's first), a per-slot done, and the compact record layout with auto_reset.

record_begin_torch / record_step_torch / record_step_done_torch and lanes_begin_torch / lanes_restart_torch /
lanes_record_torch / lanes_close_torch restate the native calls in torch ops on any device: their
executable specification and the CPU path (ExternalRollout(native=False) runs them instead of the
launches; the sampling itself has no CPU path, so the class needs the GPU either way).
"""
import ctypes

import torch

from . import _lib
from .policy import SamplingSession, noise_key
from .rollout import NF_C, RolloutBatch


def record_begin_torch(exist, compact=False):
    """mhppo_record_begin in torch ops: exist uint8 / bool [M, S] -> (ep_min float64 [M, S] of +0.0,
    rec_buf int32 [M S + M + 1] or None).  rec_buf[:M S] is rec_of (each present segment's rank in
    (row, slot) order, -1 for absent ones), rec_buf[M S:] the per-row prefix."""
    M, S = exist.shape
    ep_min = torch.zeros((M, S), dtype=torch.float64, device=exist.device)
    if not compact:
        return ep_min, None
    f = exist.reshape(-1) != 0
    incl = torch.cumsum(f.to(torch.int64), 0)
    before = incl - f.to(torch.int64)  # flagged segments before s
    rank = torch.where(f, before, torch.full_like(before, -1))
    total = incl[-1:] if M * S else torch.zeros(1, dtype=torch.int64, device=exist.device)
    pre = torch.cat([before[::S], total])
    return ep_min, torch.cat([rank, pre]).to(torch.int32)


def record_step_torch(t, act, logp, feat_c, rew, rew_light, rec_of, obs_c_tm, act_tm, logp_tm, rew_tm, ep_min):
    """mhppo_record_step in torch ops, in place on the records and ep_min: segment s of step t goes
    to record r = s (rec_of None) or rec_of[s] (none for rec_of[s] < 0) of obs_c_tm [T, M S, 13],
    act_tm / logp_tm [T, M S] and rew_tm float64 [T, M S]; ep_min takes the collector's episodic
    minimum of rew_light for every segment.  The minimum is the kernel's own expression, not
    torch.minimum (whose result for (+0.0, -0.0) is the backend's choice; the collector keeps the old value)."""
    T = act_tm.shape[0]
    if not 0 <= int(t) < T:
        raise ValueError(f"record_step_torch: t {t} outside [0, {T})")
    NS = act.numel()
    srcs = ((obs_c_tm, feat_c, NF_C), (act_tm, act, 1), (logp_tm, logp, 1), (rew_tm, rew, 1))
    if rec_of is None:
        for dst, x, w in srcs:
            dst[t].reshape(NS, w).copy_(x.reshape(NS, w))
    else:
        seg = torch.nonzero(rec_of[:NS] >= 0).squeeze(1)
        r = rec_of[:NS].index_select(0, seg).long()
        for dst, x, w in srcs:
            dst[t].reshape(NS, w).index_copy_(0, r, x.reshape(NS, w).index_select(0, seg))
    m, x = ep_min, rew_light.reshape(ep_min.shape)
    ep_min.copy_(torch.where(m != m, m, torch.where(x != x, x, torch.where(x < m, x, m))))


def record_step_done_torch(t, act, logp, feat_c, rew, rew_light, rec_of, obs_c_tm, act_tm, logp_tm, rew_tm, ep_min,
                           done, len, truncated=None, trunc=None):
    """mhppo_record_step_done in torch ops, in place: record_step_torch's records for every segment,
    finished or not; ep_min only for the segments of streams that were running on entry (len[r] == 0);
    len[r] = t + 1 for the running streams with done[r] != 0.  done bool / uint8 [M], len int32 [M].
    With truncated bool / uint8 [M] and trunc uint8 [M] (the truncation bootstrap): trunc[r] =
    truncated[r] != 0 for exactly the streams whose len this call sets -- the first done; before and
    after it truncated is ignored."""
    if (truncated is None) != (trunc is None):
        raise ValueError("record_step_done_torch: truncated and trunc go together")
    live = len == 0
    before = ep_min.clone()
    record_step_torch(t, act, logp, feat_c, rew, rew_light, rec_of, obs_c_tm, act_tm, logp_tm, rew_tm, ep_min)
    ep_min.copy_(torch.where(live[:, None], ep_min, before))
    ends = live & (done.reshape(-1) != 0)
    len.copy_(torch.where(ends, torch.full_like(len, int(t) + 1), len))
    if trunc is not None:
        trunc.copy_(torch.where(ends, (truncated.reshape(-1) != 0).to(trunc.dtype), trunc))


LANE_KEYS = ("a_d", "logp_d", "probs", "feat_d", "closest", "exist")  # mhppo_decision's arrays


def lanes_begin_torch(first, E):
    """mhppo_lanes_begin in torch ops (any device): the lanes of M streams from the window's first
    SampleDecision (with probs and feat_d) -> a dict of the mhppo_lanes arrays: the six LANE_KEYS
    lane-major [E M, ...] (lane 0 = first, every other lane 0), ep_min float64 [E M, S] of +0.0, t0 and len
    int32 [E M] of 0, cur int32 [2 M] of 0 (private: cur[(t & 1) M + r] is stream r's lane at step t)."""
    E = int(E)
    if E < 1:
        raise ValueError("lanes_begin_torch: E < 1")
    M, S = first.exist.shape
    dev = first.exist.device
    lanes = {}
    for k in LANE_KEYS:
        x = getattr(first, k)
        lanes[k] = torch.zeros((E * M,) + tuple(x.shape[1:]), dtype=x.dtype, device=dev)
        lanes[k][:M] = x
    lanes["ep_min"] = torch.zeros((E * M, S), dtype=torch.float64, device=dev)
    lanes["t0"] = torch.zeros(E * M, dtype=torch.int32, device=dev)
    lanes["len"] = torch.zeros(E * M, dtype=torch.int32, device=dev)
    lanes["cur"] = torch.zeros(2 * M, dtype=torch.int32, device=dev)
    return lanes


def _lane_shape(lanes):
    M = lanes["cur"].numel() // 2
    return lanes["t0"].numel() // max(1, M), M


def lanes_restart_torch(lanes, t, fresh, current):
    """mhppo_lanes_restart in torch ops, in place: step t >= 1, before its record.  Stream r restarts iff
    its current lane e = cur[((t - 1) & 1) M + r] is closed (len != 0) and e + 1 < E; for those streams the
    rows of the SampleDecision `fresh` go to lane e + 1 of every LANE_KEYS array and to `current` (the
    decision sample_act reads), t0 of the new lane is t, and cur[(t & 1) M + r] = e + 1 (e for the others,
    whose lanes and rows of `current` keep their bits)."""
    E, M = _lane_shape(lanes)
    t = int(t)
    if t < 1:
        raise ValueError("lanes_restart_torch: t < 1")
    r = torch.arange(M, device=lanes["cur"].device)
    e = lanes["cur"][((t - 1) & 1) * M:][:M].long()
    go = (lanes["len"][e * M + r] != 0) & (e + 1 < E)
    new = (e + 1).clamp_max(E - 1) * M + r  # one lane per stream: distinct indices
    for k in LANE_KEYS:
        f, c, a = getattr(fresh, k), getattr(current, k), lanes[k]
        g = go.reshape((M,) + (1,) * (f.dim() - 1))
        a[new] = torch.where(g, f, a[new])
        c.copy_(torch.where(g, f, c))
    lanes["t0"][new] = torch.where(go, torch.full_like(lanes["t0"][new], t), lanes["t0"][new])
    lanes["cur"][(t & 1) * M:][:M] = (e + go).to(torch.int32)


def lanes_record_torch(lanes, t, act, logp, feat_c, rew, rew_light, obs_c_tm, act_tm, logp_tm, rew_tm, done):
    """mhppo_lanes_record in torch ops, in place: record_step_torch's records of step t in the identity
    layout for every stream, idle or not; with e = cur[(t & 1) M + r] and v = e M + r, lane v runs on entry
    iff len[v] == 0: then its ep_min row takes record_step_torch's minimum, and done[r] != 0 closes it
    with len[v] = t + 1 - t0[v]."""
    E, M = _lane_shape(lanes)
    r = torch.arange(M, device=lanes["cur"].device)
    v = lanes["cur"][(int(t) & 1) * M:][:M].long() * M + r
    live = lanes["len"][v] == 0
    m = lanes["ep_min"][v]
    before = m.clone()
    record_step_torch(t, act, logp, feat_c, rew, rew_light, None, obs_c_tm, act_tm, logp_tm, rew_tm, m)
    lanes["ep_min"][v] = torch.where(live[:, None], m, before)
    ends = live & (done.reshape(-1) != 0)
    lanes["len"][v] = torch.where(ends, int(t) + 1 - lanes["t0"][v], lanes["len"][v])


def lanes_close_torch(lanes, k):
    """mhppo_lanes_close in torch ops: after k recorded steps -> (len int32 [E M], cut uint8 [E M]); a
    lane that was started (e <= cur[((k - 1) & 1) M + r]) and is still open gets len = k - t0 and cut = 1,
    every other lane its len (0 for one never started) and cut = 0.  lanes is not changed."""
    E, M = _lane_shape(lanes)
    k = int(k)
    if k < 1:
        raise ValueError("lanes_close_torch: k < 1")
    v = torch.arange(E * M, device=lanes["cur"].device)
    cur = lanes["cur"][((k - 1) & 1) * M:][:M]
    is_open = (torch.div(v, M, rounding_mode="floor") <= cur[v % M]) & (lanes["len"] == 0)
    return torch.where(is_open, k - lanes["t0"], lanes["len"]), is_open.to(torch.uint8)


class ExternalRollout:
    """One episode of M parallel streams whose rows come from a simulator outside the library.

    policy: a mhppo.policy.Policy (Algo_PPO.policy()); stream r is env first_env + r of the collector's
    Philox noise under `seed`.  compact=None: the compact record layout for the scalable variant, the
    identity layout otherwise (RolloutGPU's choice); compact=True on another variant raises.  The
    buffers are allocated once, on the policy's GPU.

        ext.begin(obs, iteration)            # the episode's first rows: the one choice of the episode
        for t in range(T):
            actions = ext.act(obs, t)        # float64 [M, 2S], the layout VecCrosswalk.step takes
            obs, rew, rew_light = ...        # the simulator's step
            ext.record(rew, rew_light)       # [M, S] device tensors
        cross, wait, choice = bucket_segments(ext.batch(), status=ext.status)

    or ext.collect(sim, iteration) for a `sim` with reset() -> obs and step(actions) -> (obs, rew,
    rew_light, ...).  By default episodes have the fixed length T: the time limit is terminal and a
    simulator's done is ignored.

    early_end=True: record(rew, rew_light, done) takes done, a bool / uint8 [M] device tensor, one flag
    per stream (all S slots of a stream share its length).  The step that first reports done is the
    stream's last (length L = t + 1) and terminal; a done raised again later is ignored, and the
    simulator may go on being stepped for finished streams: their rows are ignored.  self.len int32 [M]
    holds the lengths, 0 for a stream still running.  batch() may then be taken after any k >= 1
    recorded steps -- streams still running are cut at k, which is terminal as T is -- and carries len
    and steps = k, which send bucket_segments down its ragged path.  The policy noise is a function of
    (seed, iteration, t, env) alone, so a stream's draws do not depend on which others have ended.

    bootstrap=True (needs early_end=True): record(rew, rew_light, done, truncated) also takes truncated,
    a bool / uint8 [M] device tensor read only at the step where a running stream first reports done:
    self.trunc uint8 [M] keeps it (if a simulator raises terminated and truncated together, what it
    passes as truncated decides).  A truncated episode has not ended: bucket_segments(batch, boot=
    (critic_cross, critic_wait)) starts its segments' targets from V(s_L) instead of 0.  A stream still
    running when the batch is taken (after k recorded steps, k = T included) is cut at k, which is a
    truncation iff cut_truncates (default True: a time limit is a truncation).  The successor row s_L
    of a truncated stream of length L < k is the row handed to act(obs, L): for a truncated stream
    that row must be its true successor (Gymnasium's final_observation), not a reset row -- a
    VecCrosswalk keeps stepping finished streams without resetting and satisfies this as it is.  For
    L == k, finish(obs) takes the rows after the last recorded step; batch() without finish is legal,
    and then the streams of effective length k are not bootstrapped (v_boot = 0).  With
    cut_truncates=False and no truncated flag raised the batch's buckets are those of early_end=True
    alone, bit for bit.  The choice head's target, ep_min and the reward sums do not change.

    auto_reset=E (an integer >= 1; implies early_end's record(rew, rew_light, done)): for a simulator with
    same-step auto-reset -- after a done, the row it returns is already the new episode's first.  Stream r
    owns E lanes, lane e M + r being the e-th episode it starts in the window; lane 0 starts at step 0.  A
    done at recorded step t ends the running lane (terminal, length t + 1 - t0); if a lane is left, act(obs,
    t + 1) starts the next one at t0 = t + 1 and draws it a fresh choice decision from that row (a_d,
    logp_d, probs, feat_d, closest, exist), which sample_act uses from then on; a stream that does not
    restart keeps its decision bit for bit.  A lane is created only when act is called for its first
    step, so a done at the last recorded step opens no empty lane.  After its E-th episode a stream idles:
    its records are stored, nothing of them reaches a bucket row, a return, an ep_min or a reward sum;
    auto_reset=1 is early_end=True exactly.  The restart noise is Philox under the iteration's key at
    counter (t + 1) 2^40 + 2^39 + (first_env + r) S P + i P + p (a function of (seed, iteration, t, env)
    alone; the eps counters (t + 1) 2^40 + (first_env + r) S + i cannot reach it: (first_env + M) S P >=
    2^39 raises), or the step's tape act(obs, t, u=...) / act(obs, t, forced=...), read only for the
    restarting streams.  The re-decision runs over all M rows and may OR the NaN status for a row that
    does not restart: NaN weights flag everywhere anyway.  batch() may be taken after any k >= 1 recorded
    steps: the lanes still open are closed at k - t0 and marked cut -- terminal, or with bootstrap=True
    and finish(obs) bootstrapped from V(feat_tail) iff cut_truncates.  The batch carries the lane-major
    decisions and ep_min, lanes = E, M, t0 / len int32 [E M], cut uint8 [E M], steps = k and the wall-clock
    records, always in the identity layout (exist can differ between a stream's episodes; absent slots are
    recorded and not bucketed).  Not supported, each a ValueError: compact=True, record(..., truncated),
    and downstream gae_lambda; next-step auto-reset simulators and a per-slot done are out of scope."""

    def __init__(self, policy, M, T=80, seed=0, first_env=0, compact=None, native=True, early_end=False,
                 bootstrap=False, cut_truncates=True, auto_reset=None):
        if policy.variant == "4cars2":
            raise ValueError("4cars2 is an env-level variant only: the reference has no driver for it "
                             "(RolloutGPU refuses it too)")
        if auto_reset is not None:
            if isinstance(auto_reset, bool) or not isinstance(auto_reset, int) or auto_reset < 1:
                raise ValueError(f"ExternalRollout: auto_reset is None or an integer >= 1, not {auto_reset!r}")
            if compact:
                raise ValueError("ExternalRollout: auto_reset records in the identity layout (exist can differ "
                                 "between a stream's episodes): compact=True is not supported")
            compact, early_end = False, True
        self.lanes_E = auto_reset
        if compact is None:
            compact = policy.variant == "scalable"
        if compact and policy.variant != "scalable":
            raise ValueError("the compact record layout is the scalable variant's (the one whose car slots can be absent)")
        M, T = int(M), int(T)
        if M < 0 or T < 1:
            raise ValueError(f"ExternalRollout needs M >= 0 and T >= 1, not M = {M}, T = {T}")
        self.policy, self.M, self.T, self.native, self.compact = policy, M, T, bool(native), bool(compact)
        self.early_end, self.bootstrap, self.cut_truncates = bool(early_end), bool(bootstrap), bool(cut_truncates)
        if self.bootstrap and not self.early_end:
            raise ValueError("ExternalRollout: bootstrap=True needs early_end=True")
        self.N, self.S, self.P = M, policy.n_slots, policy.nb_ped
        if M * self.S > 2**31 - 1:
            raise ValueError("ExternalRollout: M S > 2^31 - 1")
        if auto_reset is not None and auto_reset * M * self.S > 2**31 - 1:
            raise ValueError("ExternalRollout: auto_reset M S > 2^31 - 1")
        self.session = SamplingSession(policy, M, seed=seed, first_env=first_env)
        if auto_reset is not None:
            self._restart_offset(1)
        dev = policy.actor_choice.flat().device
        if dev.type != "cuda":
            raise ValueError("ExternalRollout runs on the nets' GPU (the sampling has no CPU path)")
        self.device = dev
        S = self.S
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.obs_c = z((T, M, S, NF_C), torch.float32)
        self.act_tm = z((T, M, S), torch.float32)
        self.logp_tm = z((T, M, S), torch.float32)
        self.rew_tm = z((T, M, S), torch.float64)
        self.ep_min = z((M, S), torch.float64)
        self.rec_buf = z(M * S + M + 1, torch.int32) if self.compact else None  # segment ranks | per-row prefix
        self.rec_of = self.rec_buf[:M * S] if self.compact else None
        # the streams' lengths, 0: still running (auto_reset: the lanes' len instead, self.lanes["len"])
        self.len = z(M, torch.int32) if self.early_end and auto_reset is None else None
        self.lanes = None  # auto_reset: the mhppo_lanes arrays (lanes_begin_torch's dict), made by begin()
        self.trunc = z(M, torch.uint8) if self.bootstrap else None  # the first done was a truncation
        self.feat_tail = None  # finish(): the features of the rows after the last recorded step, [M, S, 13]
        self.status = z(1, torch.int32)  # NaN flags of the policy draws, for bucket_segments(status=...)
        self._work = z(max(1, int(_lib.lib().mhppo_record_work_bytes(M, S)) // 8), torch.float64)
        self._t = None        # the step act() was last called for
        self._recorded = -1   # the last step recorded
        self._begun = False

    def _st(self):
        return _lib.stream_ptr(device=self.device)

    def _restart_offset(self, t):
        """The Philox counter of step t's restart uniforms for stream 0, checked against the eps counters."""
        s = self.session
        if (s.first_env + self.M) * self.S * self.P >= 2**39:
            raise ValueError("ExternalRollout: auto_reset needs (first_env + M) S P < 2^39 (the restart counters)")
        return ((int(t) + 1) << 40) + (1 << 39) + s.first_env * self.S * self.P

    def _lanes_struct(self):
        a = self.lanes
        d = _lib.Decision(*[a[k].data_ptr() for k in LANE_KEYS])
        return _lib.Lanes(d, a["ep_min"].data_ptr(), a["t0"].data_ptr(), a["len"].data_ptr(), a["cur"].data_ptr())

    @staticmethod
    def _decision_struct(d):
        return _lib.Decision(*[getattr(d, k).data_ptr() for k in LANE_KEYS])

    def _lanes_begin(self, d):
        E, M, S, P = self.lanes_E, self.M, self.S, self.P
        if not self.native:
            self.lanes = lanes_begin_torch(d, E)
            return
        if self.lanes is None:  # allocated once; mhppo_lanes_begin writes every element
            e = lambda x: torch.empty((E * M,) + tuple(x.shape[1:]), dtype=x.dtype, device=self.device)
            self.lanes = {k: e(getattr(d, k)) for k in LANE_KEYS}
            self.lanes.update(ep_min=e(self.ep_min), t0=torch.empty(E * M, dtype=torch.int32, device=self.device),
                              len=torch.empty(E * M, dtype=torch.int32, device=self.device),
                              cur=torch.empty(2 * M, dtype=torch.int32, device=self.device))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mhppo_lanes_begin(ctypes.byref(self._lanes_struct()), E, M, S, P, d.feat_d.shape[-1],
                                                    ctypes.byref(self._decision_struct(d)), self._st()))

    def _lanes_restart(self, obs, t, u, forced):
        """auto_reset, step t >= 1: the fresh decision of every row (Philox at the restart counters, or
        the step's tape) and its merge into the restarting streams' new lane and the decision in force."""
        s = self.session
        if u is None and forced is None:
            u = torch.empty((self.M, self.S, self.P), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().mhppo_philox_uniform(s.key, self._restart_offset(t), _lib.ptr(u), u.numel(),
                                                           self._st()))
        fresh = self.policy.sample_decide(obs, u=u, forced=forced, want_probs=True, want_features=True,
                                          status=self.status)
        if not self.native:
            lanes_restart_torch(self.lanes, t, fresh, s.decision)
            return
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mhppo_lanes_restart(
                ctypes.byref(self._lanes_struct()), self.lanes_E, self.M, self.S, self.P, fresh.feat_d.shape[-1], t,
                self.T, ctypes.byref(self._decision_struct(fresh)), ctypes.byref(self._decision_struct(s.decision)),
                self._st()))

    def begin(self, obs, iteration, u=None, forced=None):
        """Start an episode on its first rows obs float32 [M, obs_dim]: the status word is zeroed, the
        choice of every (slot, pedestrian) is drawn -- Philox at the collector's counters of (seed,
        iteration), or from the tape u float32 [M, S, P] / the decisions forced int32 [M, S, P] -- and
        the records begin.  Returns the SampleDecision."""
        s = self.session
        s._check(obs, "begin")
        self.status.zero_()
        s.key = noise_key(s.seed, iteration)
        if u is None and forced is None:
            d = s.begin(obs, iteration, want_probs=True, want_features=True, status=self.status)
        else:
            d = s.decision = self.policy.sample_decide(obs, u=u, forced=forced, want_probs=True, want_features=True,
                                                       status=self.status)
        if self.lanes_E is not None:
            self._lanes_begin(d)
        elif self.native:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().mhppo_record_begin(_lib.ptr(d.exist), self.M, self.S, _lib.ptr(self.rec_buf),
                                                         _lib.ptr(self.ep_min), _lib.ptr(self._work), self._st()))
        else:
            ep_min, rec = record_begin_torch(d.exist, self.compact)
            self.ep_min.copy_(ep_min)
            if self.compact:
                self.rec_buf.copy_(rec)
        if self.len is not None:
            self.len.zero_()
        if self.bootstrap:
            self.trunc.zero_()
        self.feat_tail = None
        self._t, self._recorded, self._begun = None, -1, True
        return d

    def act(self, obs, t, eps=None, u=None, forced=None):
        """actions float64 [M, 2S] for step t's rows (SamplingSession.step; eps float32 [M, S]: the
        tape form of Policy.sample_act instead of the Philox draw).  With auto_reset, steps are acted on
        once each, in order, and at t >= 1 the streams whose episode ended at step t - 1 and that have a lane
        left first draw their new episode's choice decision from this row: Philox at the restart
        counters, or the step's tape u float32 / forced int32 [M, S, P] (read only for restarting streams;
        without auto_reset either raises).  The re-decision covers all M rows and may OR the NaN status
        for a row that does not restart."""
        if not self._begun:
            raise ValueError("ExternalRollout.act before begin")
        t = int(t)
        if not 0 <= t < self.T:
            raise ValueError(f"ExternalRollout.act: t {t} outside [0, {self.T})")
        s = self.session
        if self.lanes_E is None:
            if u is not None or forced is not None:
                raise ValueError("ExternalRollout.act takes u / forced with auto_reset only")
        else:
            if u is not None and forced is not None:
                raise ValueError("ExternalRollout.act takes one restart tape: u or forced")
            if self.feat_tail is not None:
                raise ValueError("ExternalRollout.act after finish")
            if t != self._recorded + 1 or self._t == t:
                raise ValueError(f"ExternalRollout.act: step {t} after step {self._recorded} was recorded: with "
                                 "auto_reset steps are acted on once each, in order")
            s._check(obs, "step")
            if t >= 1 and self.lanes_E > 1:  # E == 1: nothing can restart
                self._lanes_restart(obs, t, u, forced)
        if eps is None:
            actions = s.step(obs, t, status=self.status)
        else:
            s._check(obs, "step")
            r = self.policy.sample_act(obs, s.decision.a_d, s.decision.closest, eps=eps, status=self.status)
            s.act, s.logp, s.feat_c, actions = r.act, r.logp, r.feat_c, r.actions
        self._t = t
        return actions

    def _flags(self, x, name):
        if (not torch.is_tensor(x) or tuple(x.shape) != (self.M,) or x.device != self.device
                or x.dtype not in (torch.bool, torch.uint8)):
            raise ValueError(f"ExternalRollout.record takes {name} as a bool or uint8 [{self.M}] tensor on {self.device}")
        x = x.detach().contiguous()
        return x.view(torch.uint8) if x.dtype == torch.bool else x

    def record(self, rew, rew_light, done=None, truncated=None):
        """Record the step act() was last called for with the simulator's rew / rew_light, [M, S] tensors
        on the device (converted to float64).  Steps are recorded once each, in order from 0.  With
        early_end the step's done, a bool / uint8 [M] tensor on the device, is required; without it,
        passing done raises.  With bootstrap the step's truncated, of the same form, is required too
        (read only where a running stream first reports done); without it, passing truncated raises."""
        if self._t is None:
            raise ValueError("ExternalRollout.record before act")
        if self.feat_tail is not None:
            raise ValueError("ExternalRollout.record after finish")
        if self._t == self._recorded:
            raise ValueError(f"ExternalRollout.record: step {self._t} is recorded already")
        if self._t != self._recorded + 1:
            raise ValueError(f"ExternalRollout.record: step {self._t} after step {self._recorded}: steps are "
                             "recorded in order")
        for name, x in (("rew", rew), ("rew_light", rew_light)):
            if (not torch.is_tensor(x) or tuple(x.shape) != (self.M, self.S) or x.device != self.device
                    or not x.is_floating_point()):
                raise ValueError(f"ExternalRollout.record takes {name} as a floating-point [{self.M}, {self.S}] "
                                 f"tensor on {self.device}")
        if not self.early_end and done is not None:
            raise ValueError("ExternalRollout.record takes done with early_end=True only")
        if not self.bootstrap and truncated is not None:
            raise ValueError("ExternalRollout.record takes truncated with bootstrap=True only")
        if self.lanes_E is not None and truncated is not None:
            raise ValueError("ExternalRollout.record takes no truncated with auto_reset: a mid-window truncation "
                             "needs the simulator's final observation (out of scope)")
        if self.early_end:
            done = self._flags(done, "done")
        if self.bootstrap and self.lanes_E is None:
            truncated = self._flags(truncated, "truncated")
        rew = rew.detach().to(torch.float64).contiguous()
        rew_light = rew_light.detach().to(torch.float64).contiguous()
        s, t = self.session, self._t
        if self.lanes_E is not None:
            if self.native:
                p = _lib.ptr
                with torch.cuda.device(self.device):
                    _lib.check(_lib.lib().mhppo_lanes_record(
                        ctypes.byref(self._lanes_struct()), self.lanes_E, self.M, self.S, t, self.T, p(s.act), p(s.logp),
                        p(s.feat_c), p(rew), p(rew_light), p(self.obs_c), p(self.act_tm), p(self.logp_tm),
                        p(self.rew_tm), p(done), self._st()))
            else:
                NS = self.M * self.S
                lanes_record_torch(self.lanes, t, s.act, s.logp, s.feat_c, rew, rew_light,
                                   self.obs_c.view(self.T, NS, NF_C), self.act_tm.view(self.T, NS),
                                   self.logp_tm.view(self.T, NS), self.rew_tm.view(self.T, NS), done)
        elif self.native:
            if self.bootstrap:  # the streams whose len the launch below sets: their first done
                ends = (self.len == 0) & (done != 0)
                self.trunc.copy_(torch.where(ends, (truncated != 0).to(torch.uint8), self.trunc))
            p = _lib.ptr
            args = (self.M, self.S, t, self.T, p(s.act), p(s.logp), p(s.feat_c), p(rew), p(rew_light), p(self.rec_of),
                    p(self.obs_c), p(self.act_tm), p(self.logp_tm), p(self.rew_tm), p(self.ep_min))
            with torch.cuda.device(self.device):
                if self.early_end:
                    _lib.check(_lib.lib().mhppo_record_step_done(*args, p(done), p(self.len), self._st()))
                else:
                    _lib.check(_lib.lib().mhppo_record_step(*args, self._st()))
        else:
            NS = self.M * self.S
            recs = (self.obs_c.view(self.T, NS, NF_C), self.act_tm.view(self.T, NS), self.logp_tm.view(self.T, NS),
                    self.rew_tm.view(self.T, NS), self.ep_min)
            if self.early_end:
                record_step_done_torch(t, s.act, s.logp, s.feat_c, rew, rew_light, self.rec_of, *recs, done, self.len,
                                       truncated, self.trunc)
            else:
                record_step_torch(t, s.act, s.logp, s.feat_c, rew, rew_light, self.rec_of, *recs)
        self._recorded = t

    def finish(self, obs):
        """bootstrap only: obs float32 [M, obs_dim], the rows after the last recorded step, so that the
        streams of effective length k (cut, or ended at the last step by a truncation) can be
        bootstrapped.  Runs Policy.sample_act on them with the episode's decision and a zero eps tape --
        the feature rows depend on the observation and the decision alone -- and keeps only feat_c, as
        self.feat_tail float32 [M, S, 13] in segment layout; the actions and log-probs are discarded.
        Once per episode, after at least one recorded step; no record after it."""
        if not self.bootstrap:
            raise ValueError("ExternalRollout.finish needs bootstrap=True")
        if not self._begun or self._recorded < 0:
            raise ValueError("ExternalRollout.finish before any step is recorded")
        if self.feat_tail is not None:
            raise ValueError("ExternalRollout.finish was called already")
        s = self.session
        s._check(obs, "finish")
        eps = torch.zeros((self.M, self.S), dtype=torch.float32, device=self.device)
        r = self.policy.sample_act(obs, s.decision.a_d, s.decision.closest, eps=eps)  # no status: nothing is sampled
        self.feat_tail = r.feat_c.reshape(self.M, self.S, NF_C)

    def batch(self):
        """The RolloutBatch of the episode, with the fields RolloutGPU.collect returns (N = M); with
        early_end, after any k >= 1 recorded steps, also len (int32 [M]) and steps = k; with bootstrap
        also trunc (uint8 [M]), feat_tail (float32 [M, S, 13], or None without finish: the streams of
        effective length k are then not bootstrapped) and cut_truncates."""
        if not self._begun or (self._recorded < 0 if self.early_end else self._recorded != self.T - 1):
            raise ValueError(f"ExternalRollout.batch: {self._recorded + 1} of {self.T} steps recorded")
        if self.lanes_E is not None:
            return self._lanes_batch()
        d = self.session.decision
        ragged = dict(len=self.len, steps=self._recorded + 1) if self.early_end else {}
        if self.bootstrap:
            ragged.update(trunc=self.trunc, feat_tail=self.feat_tail, cut_truncates=self.cut_truncates)
        views = {} if self.compact else dict(obs_c=self.obs_c.permute(1, 2, 0, 3), act=self.act_tm.permute(1, 2, 0),
                                             logp=self.logp_tm.permute(1, 2, 0), rew=self.rew_tm.permute(1, 2, 0))
        return RolloutBatch(feat_d=d.feat_d, probs_d=d.probs, logp_d=d.logp_d, a_d=d.a_d, closest=d.closest, **views,
                            obs_c_tm=self.obs_c, act_tm=self.act_tm, logp_tm=self.logp_tm, rew_tm=self.rew_tm,
                            ep_min=self.ep_min, rec_of=self.rec_of, exist=d.exist, N=self.M, S=self.S, P=self.P,
                            T=self.T, **ragged)

    def _lanes_batch(self):
        """batch() with auto_reset: the lane-major decisions and ep_min, the wall-clock records, lanes = E,
        M, t0 / len int32 [E M] and cut uint8 [E M] (mhppo_lanes_close: the lanes still open are cut at
        k - t0; the lanes themselves are not changed, recording may go on), steps = k, feat_tail and
        cut_truncates.  trunc is not set."""
        if self._t != self._recorded:
            raise ValueError(f"ExternalRollout.batch: step {self._t} was acted on and not recorded")
        E, M, k, a = self.lanes_E, self.M, self._recorded + 1, self.lanes
        if self.native:
            ln = torch.empty(E * M, dtype=torch.int32, device=self.device)
            cut = torch.empty(E * M, dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().mhppo_lanes_close(ctypes.byref(self._lanes_struct()), E, M, k, self.T, _lib.ptr(ln),
                                                        _lib.ptr(cut), self._st()))
        else:
            ln, cut = lanes_close_torch(a, k)
        return RolloutBatch(feat_d=a["feat_d"], probs_d=a["probs"], logp_d=a["logp_d"], a_d=a["a_d"],
                            closest=a["closest"], exist=a["exist"], ep_min=a["ep_min"],
                            obs_c=self.obs_c.permute(1, 2, 0, 3), act=self.act_tm.permute(1, 2, 0),
                            logp=self.logp_tm.permute(1, 2, 0), rew=self.rew_tm.permute(1, 2, 0),
                            obs_c_tm=self.obs_c, act_tm=self.act_tm, logp_tm=self.logp_tm, rew_tm=self.rew_tm,
                            rec_of=None, N=M, M=M, S=self.S, P=self.P, T=self.T, lanes=E, t0=a["t0"], len=ln, cut=cut,
                            steps=k, feat_tail=self.feat_tail, cut_truncates=self.cut_truncates)

    def collect(self, sim, iteration, check_every=None):
        """The episode loop on `sim`: anything with reset() -> obs and step(actions) -> (obs, rew,
        rew_light, ...) returning device tensors (a VecCrosswalk qualifies as it is).  With early_end the
        step's fourth value is the streams' done, with bootstrap its fifth their truncated, and finish()
        gets the rows the last step returned.  check_every=n (early_end only): every n steps the host
        reads whether every stream has ended and stops the episode if so; None: no host read, T steps.
        With auto_reset the fourth value is done, there is no fifth, and check_every stops once every
        stream is idle (its E-th episode has ended)."""
        if check_every is not None:
            if not self.early_end:
                raise ValueError("ExternalRollout.collect: check_every needs early_end=True")
            if isinstance(check_every, bool) or not isinstance(check_every, int) or check_every < 1:
                raise ValueError(f"ExternalRollout.collect: check_every is None or an integer >= 1, not {check_every!r}")
        with torch.no_grad():
            obs = sim.reset()
            self.begin(obs, iteration)
            for t in range(self.T):
                actions = self.act(obs, t)
                if self.lanes_E is not None:
                    obs, rew, rew_light, done, *_ = sim.step(actions)
                    self.record(rew, rew_light, done)
                    if (check_every is not None and (t + 1) % check_every == 0
                            and bool((self.lanes["len"][(self.lanes_E - 1) * self.M:] != 0).all())):
                        break
                elif self.early_end:
                    if self.bootstrap:
                        obs, rew, rew_light, done, truncated, *_ = sim.step(actions)
                        self.record(rew, rew_light, done, truncated)
                    else:
                        obs, rew, rew_light, done, *_ = sim.step(actions)
                        self.record(rew, rew_light, done)
                    if check_every is not None and (t + 1) % check_every == 0 and bool((self.len != 0).all()):
                        break
                else:
                    obs, rew, rew_light, *_ = sim.step(actions)
                    self.record(rew, rew_light)
            if self.bootstrap:
                self.finish(obs)
        return self.batch()
