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
finish(obs) for L == k.  Out of scope: auto-reset or several episodes per stream and iteration (the
choice head is one decision per episode) and a per-slot done.

record_begin_torch / record_step_torch / record_step_done_torch restate the native calls in torch ops on
any device: their executable specification and the CPU path (ExternalRollout(native=False) runs them
instead of the launches; the sampling itself has no CPU path, so the class needs the GPU either way).
"""
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
    alone, bit for bit.  The choice head's target, ep_min and the reward sums do not change."""

    def __init__(self, policy, M, T=80, seed=0, first_env=0, compact=None, native=True, early_end=False,
                 bootstrap=False, cut_truncates=True):
        if policy.variant == "4cars2":
            raise ValueError("4cars2 is an env-level variant only: the reference has no driver for it "
                             "(RolloutGPU refuses it too)")
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
        self.session = SamplingSession(policy, M, seed=seed, first_env=first_env)
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
        self.len = z(M, torch.int32) if self.early_end else None  # the streams' lengths, 0: still running
        self.trunc = z(M, torch.uint8) if self.bootstrap else None  # the first done was a truncation
        self.feat_tail = None  # finish(): the features of the rows after the last recorded step, [M, S, 13]
        self.status = z(1, torch.int32)  # NaN flags of the policy draws, for bucket_segments(status=...)
        self._work = z(max(1, int(_lib.lib().mhppo_record_work_bytes(M, S)) // 8), torch.float64)
        self._t = None        # the step act() was last called for
        self._recorded = -1   # the last step recorded
        self._begun = False

    def _st(self):
        return _lib.stream_ptr(device=self.device)

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
        if self.native:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().mhppo_record_begin(_lib.ptr(d.exist), self.M, self.S, _lib.ptr(self.rec_buf),
                                                         _lib.ptr(self.ep_min), _lib.ptr(self._work), self._st()))
        else:
            ep_min, rec = record_begin_torch(d.exist, self.compact)
            self.ep_min.copy_(ep_min)
            if self.compact:
                self.rec_buf.copy_(rec)
        if self.early_end:
            self.len.zero_()
        if self.bootstrap:
            self.trunc.zero_()
        self.feat_tail = None
        self._t, self._recorded, self._begun = None, -1, True
        return d

    def act(self, obs, t, eps=None):
        """actions float64 [M, 2S] for step t's rows (SamplingSession.step; eps float32 [M, S]: the
        tape form of Policy.sample_act instead of the Philox draw)."""
        if not self._begun:
            raise ValueError("ExternalRollout.act before begin")
        t = int(t)
        if not 0 <= t < self.T:
            raise ValueError(f"ExternalRollout.act: t {t} outside [0, {self.T})")
        s = self.session
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
        if self.early_end:
            done = self._flags(done, "done")
        if self.bootstrap:
            truncated = self._flags(truncated, "truncated")
        rew = rew.detach().to(torch.float64).contiguous()
        rew_light = rew_light.detach().to(torch.float64).contiguous()
        s, t = self.session, self._t
        if self.native:
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

    def collect(self, sim, iteration, check_every=None):
        """The episode loop on `sim`: anything with reset() -> obs and step(actions) -> (obs, rew,
        rew_light, ...) returning device tensors (a VecCrosswalk qualifies as it is).  With early_end the
        step's fourth value is the streams' done, with bootstrap its fifth their truncated, and finish()
        gets the rows the last step returned.  check_every=n (early_end only): every n steps the host
        reads whether every stream has ended and stops the episode if so; None: no host read, T steps."""
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
                if self.early_end:
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
