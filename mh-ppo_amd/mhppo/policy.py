"""Stateless policy inference: hybrid actions from observation rows, without an env.

`Policy` applies the three trained heads to float32 observation rows from anywhere (another
simulator, a recorded trajectory, a grid of observations for a decision map) on the native path
(mhppo_policy_decide / mhppo_policy_act, include/mhppo.h): the deterministic rule of the evaluation
(Env_rollout.iterations, Coop-MH-PPO-scalable.py:152-252), bit for bit what mhppo_eval_step hands
its env step.  `PolicySession` adds the evaluation's decision schedule for parallel streams of
observations.  There is no CPU path.

sample_decide / sample_act apply the TRAINING policy instead (mhppo_policy_sample_decide / _sample_act):
the collector's Categorical and Gaussian draws with their log-probabilities and recorded feature rows,
bit for bit what RolloutGPU.collect records for the same rows, weights and noise.  `SamplingSession`
strings them into the collector's episode schedule (one decision at t = 0).
"""
import ctypes

import torch

from . import _lib
from .env import CAR_B, VARIANTS, _flat

MAX_P = 32  # mhppo_policy_act: a slot's pedestrians share one 32-row tile
_MASK64 = (1 << 64) - 1


def noise_key(seed, iteration):
    """The Philox key of the collector's noise for (seed, iteration) (RolloutGPU.draw_noise)."""
    return (int(seed) * 1000003 + int(iteration)) & _MASK64


class SampleDecision:
    """Policy.sample_decide's result: a_d int32, logp_d float32 [M, S, P]; closest int32, exist uint8
    [M, S]; probs float32 [M, S, P, 2] and feat_d float32 [M, S, P, choice_dim] when asked for, else None."""

    def __init__(self, a_d, logp_d, closest, exist, probs=None, feat_d=None):
        self.a_d, self.logp_d, self.closest, self.exist, self.probs, self.feat_d = a_d, logp_d, closest, exist, probs, feat_d


class SampleAction:
    """Policy.sample_act's result: actions float64 [M, 2S] (the layout VecCrosswalk.step takes), act and
    logp float32 [M, S], feat_c float32 [M, S, 13] (None without want_features)."""

    def __init__(self, actions, act, logp, feat_c=None):
        self.actions, self.act, self.logp, self.feat_c = actions, act, logp, feat_c


class Policy:
    """The deterministic hybrid policy of one env configuration on three live nets.

    decide(obs) -> a_d int32 [M, S, P], the choice of every (slot, pedestrian);
    act(obs, a_d) -> float64 [M, 2S] = [acc.., light..], the layout VecCrosswalk.step takes.
    The nets' weights are read at every call, so a policy built on nets in training tracks them."""

    def __init__(self, variant, nb_car, nb_ped, nb_lines, actor_cross, actor_wait, actor_choice, dt=0.3, car_b=CAR_B):
        if variant not in VARIANTS:
            raise ValueError(f"unknown variant {variant!r} (one of {sorted(VARIANTS)})")
        cfg = _lib.EnvCfg()
        cfg.variant = VARIANTS[variant]
        cfg.n_envs, cfg.max_episode = 1, 80  # ignored by the policy entry points
        cfg.nb_car, cfg.nb_ped, cfg.nb_lines = int(nb_car), int(nb_ped), int(nb_lines)
        cfg.dt = float(dt)
        for i, v in enumerate(_flat(car_b, 4)):
            cfg.car_b[i] = v
        self.cfg, self.variant = cfg, variant
        dims = (ctypes.c_int32 * 4)()
        _lib.check(_lib.lib().mhppo_policy_dims(ctypes.byref(cfg), dims))
        self.obs_dim, self.n_slots, self.nb_ped, self.choice_dim = (int(x) for x in dims)
        if self.nb_ped > MAX_P:
            raise ValueError(f"nb_ped {self.nb_ped} > {MAX_P}: a slot's pedestrians must fit one 32-row tile")
        # the re-decision test reads obs[:, env_off + 1] (PolicySession): the env block sits before the pedestrians
        self.env_off = self.obs_dim - 9 * self.nb_ped - (4 if variant == "scalable" else 3)
        for name, net, kind, n_in, n_out in (("actor_cross", actor_cross, 1, 13, 1), ("actor_wait", actor_wait, 1, 13, 1),
                                             ("actor_choice", actor_choice, 2, self.choice_dim, 2)):
            if getattr(net, "model_type", None) != kind:
                raise ValueError(f"{name} must be a Model_PPO of model_type {kind} "
                                 f"({'a continuous' if kind == 1 else 'the choice'} actor), not "
                                 f"{getattr(net, 'model_type', None)}")
            if net.n_in != n_in or net.n_out != n_out:
                raise ValueError(f"{name} must be {n_in} -> {n_out} for this configuration, not {net.n_in} -> {net.n_out}")
        self.actor_cross, self.actor_wait, self.actor_choice = actor_cross, actor_wait, actor_choice

    @classmethod
    def from_env(cls, venv, actor_cross, actor_wait, actor_choice):
        """The policy of a VecCrosswalk's configuration (its dt and car bounds)."""
        c = venv.cfg
        return cls(venv.variant, venv.nb_car, venv.nb_ped, venv.nb_lines, actor_cross, actor_wait, actor_choice,
                   dt=float(c.dt), car_b=[float(x) for x in c.car_b])

    def _rows(self, obs, what):
        if not torch.is_tensor(obs) or obs.dtype != torch.float32 or obs.dim() != 2 or obs.shape[1] != self.obs_dim:
            raise ValueError(f"{what} takes a float32 [M, {self.obs_dim}] tensor of observation rows")
        dev = self.actor_choice.flat().device
        if obs.device.type != "cuda" or obs.device != dev:
            raise ValueError(f"{what} runs on the nets' GPU: obs must live there (there is no CPU path)")
        for net in (self.actor_cross, self.actor_wait):
            if net.flat().device != dev:
                raise ValueError("the three nets must live on one GPU")
        return obs.detach().contiguous()

    def decide(self, obs, probs=False):
        """a_d int32 [M, S, P]; with probs=True also the choice probabilities float32 [M, S, P, 2]."""
        obs = self._rows(obs, "Policy.decide")
        M, S, P = obs.shape[0], self.n_slots, self.nb_ped
        a_d = torch.empty((M, S, P), dtype=torch.int32, device=obs.device)
        pr = torch.empty((M, S, P, 2), dtype=torch.float32, device=obs.device) if probs else None
        d, keep = self.actor_choice.mlp_desc()
        with torch.cuda.device(obs.device):
            _lib.check(_lib.lib().mhppo_policy_decide(ctypes.byref(self.cfg), ctypes.byref(d), _lib.ptr(obs), M,
                                                      _lib.ptr(a_d), _lib.ptr(pr), _lib.stream_ptr()))
        return (a_d, pr) if probs else a_d

    def act(self, obs, a_d):
        """actions float64 [M, 2S] from the rows and their decisions a_d int32 [M, S, P]."""
        obs = self._rows(obs, "Policy.act")
        M, S, P = obs.shape[0], self.n_slots, self.nb_ped
        if (not torch.is_tensor(a_d) or a_d.dtype != torch.int32 or tuple(a_d.shape) != (M, S, P)
                or a_d.device != obs.device):
            raise ValueError(f"Policy.act takes a_d as an int32 [{M}, {S}, {P}] tensor on obs's device")
        a_d = a_d.contiguous()
        out = torch.empty((M, 2 * S), dtype=torch.float64, device=obs.device)
        dc, kc = self.actor_cross.mlp_desc()
        dw, kw = self.actor_wait.mlp_desc()
        with torch.cuda.device(obs.device):
            _lib.check(_lib.lib().mhppo_policy_act(ctypes.byref(self.cfg), ctypes.byref(dc), ctypes.byref(dw),
                                                   _lib.ptr(obs), _lib.ptr(a_d), M, _lib.ptr(out), _lib.stream_ptr()))
        return out

    def _status(self, status, dev, what):
        if status is None:
            return None
        if (not torch.is_tensor(status) or status.dtype != torch.int32 or status.numel() != 1 or status.device != dev
                or not status.is_contiguous()):
            raise ValueError(f"{what} takes status as an int32 [1] tensor on obs's device")
        return status

    def _tape(self, x, shape, dtype, dev, what, name):
        if not torch.is_tensor(x) or x.dtype != dtype or tuple(x.shape) != shape or x.device != dev:
            raise ValueError(f"{what} takes {name} as a {str(dtype).split('.')[-1]} {list(shape)} tensor on obs's device")
        return x.contiguous()

    def sample_decide(self, obs, u=None, forced=None, key=None, first_env=0, want_probs=False, want_features=False,
                      status=None):
        """The collector's Categorical draw of every (slot, pedestrian) -> SampleDecision.  Exactly one
        noise source: u float32 [M, S, P] (a_d = u >= p(cross)), forced int32 [M, S, P] (the decisions
        themselves), or key (noise_key(seed, iteration): Philox at the collector's counters, row r being
        env first_env + r).  status: int32 [1] that receives bit 1 on NaN probabilities (OR-ed in; None:
        nothing is written)."""
        what = "Policy.sample_decide"
        obs = self._rows(obs, what)
        if sum(x is not None for x in (u, forced, key)) != 1:
            raise ValueError(f"{what} takes exactly one noise source: u, forced or key")
        M, S, P = obs.shape[0], self.n_slots, self.nb_ped
        dev = obs.device
        nz = _lib.PolicyNoise()
        if u is not None:
            u = self._tape(u, (M, S, P), torch.float32, dev, what, "u")
            nz.tape = u.data_ptr()
        elif forced is not None:
            forced = self._tape(forced, (M, S, P), torch.int32, dev, what, "forced")
            nz.forced = forced.data_ptr()
        else:
            nz.key, nz.first_env = int(key) & _MASK64, int(first_env) & _MASK64
        status = self._status(status, dev, what)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = SampleDecision(e((M, S, P), torch.int32), e((M, S, P), torch.float32), e((M, S), torch.int32),
                             e((M, S), torch.uint8), e((M, S, P, 2), torch.float32) if want_probs else None,
                             e((M, S, P, self.choice_dim), torch.float32) if want_features else None)
        d, keep = self.actor_choice.mlp_desc()
        p = _lib.ptr
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mhppo_policy_sample_decide(
                ctypes.byref(self.cfg), ctypes.byref(d), p(obs), M, ctypes.byref(nz), p(out.a_d), p(out.logp_d),
                p(out.probs), p(out.feat_d), p(out.closest), p(out.exist), p(status), _lib.stream_ptr()))
        return out

    def sample_act(self, obs, a_d, closest, eps=None, key=None, first_env=0, t=0, want_features=True, status=None):
        """The collector's Gaussian draw of every slot from the rows, their decisions a_d int32 [M, S, P]
        and closest int32 [M, S] -> SampleAction.  Exactly one noise source: eps float32 [M, S] (standard
        normals), or key (Philox at the collector's counters of step t, row r being env first_env + r).
        status: int32 [1] that receives bit 2 on a NaN loc."""
        what = "Policy.sample_act"
        obs = self._rows(obs, what)
        if sum(x is not None for x in (eps, key)) != 1:
            raise ValueError(f"{what} takes exactly one noise source: eps or key")
        M, S, P = obs.shape[0], self.n_slots, self.nb_ped
        dev = obs.device
        a_d = self._tape(a_d, (M, S, P), torch.int32, dev, what, "a_d")
        closest = self._tape(closest, (M, S), torch.int32, dev, what, "closest")
        nz = _lib.PolicyNoise()
        if eps is not None:
            eps = self._tape(eps, (M, S), torch.float32, dev, what, "eps")
            nz.tape = eps.data_ptr()
        else:
            if int(t) < 0:
                raise ValueError(f"{what}: t < 0")
            nz.key, nz.first_env, nz.t = int(key) & _MASK64, int(first_env) & _MASK64, int(t)
        status = self._status(status, dev, what)
        e = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        out = SampleAction(e((M, 2 * S), torch.float64), e((M, S), torch.float32), e((M, S), torch.float32),
                           e((M, S, 13), torch.float32) if want_features else None)
        dc, kc = self.actor_cross.mlp_desc()
        dw, kw = self.actor_wait.mlp_desc()
        p = _lib.ptr
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().mhppo_policy_sample_act(
                ctypes.byref(self.cfg), ctypes.byref(dc), ctypes.byref(dw), p(obs), p(a_d), p(closest), M,
                ctypes.byref(nz), p(out.actions), p(out.act), p(out.logp), p(out.feat_c), p(status),
                _lib.stream_ptr()))
        return out


class PolicySession:
    """The evaluation's decision schedule for M parallel streams of observations.

    step(obs, start=None) -> actions [M, 2S] for this call's row of every stream.  A stream's choice is
    re-decided where `start` (True, or bool [M]) is set — at the first call everywhere — and where
    the evaluation's re-decision test fires between the previous call's observation and this one
    (c = obs[:, env_off + 1]: c != nb_ped for the scalable variant, c != the previous c otherwise);
    elsewhere the stream keeps its choice.  Device ops only, no host read."""

    def __init__(self, policy, M):
        self.policy, self.M = policy, int(M)
        self.a_d = None     # the choices in force, int32 [M, S, P]
        self.c_prev = None  # obs[:, env_off + 1] of the previous call

    def step(self, obs, start=None):
        pol = self.policy
        if torch.is_tensor(obs) and obs.dim() == 2 and obs.shape[0] != self.M:
            raise ValueError(f"PolicySession.step takes one row per stream: [{self.M}, {pol.obs_dim}]")
        a_new = pol.decide(obs)
        c = obs[:, pol.env_off + 1].clone()
        if self.a_d is None:  # the first call decides for every stream, whatever `start` says
            self.a_d = a_new
        else:
            due = (c != float(pol.nb_ped)) if pol.variant == "scalable" else (c != self.c_prev)
            if start is not None:
                s = torch.as_tensor(start, dtype=torch.bool, device=obs.device)
                due = due | (s.expand(self.M) if s.dim() == 0 else s)
            self.a_d = torch.where(due[:, None, None], a_new, self.a_d)
        self.c_prev = c
        return pol.act(obs, self.a_d)


class SamplingSession:
    """The collector's episode schedule for M parallel streams, env first_env + r being stream r, under
    the collector's Philox noise of `seed`: begin(obs, iteration) decides once from the episode's first
    rows (the collector decides at t = 0 only), step(obs, t) -> actions [M, 2S] for step t's rows and keeps
    that step's act, logp and feat_c.  Device ops only, no host read."""

    def __init__(self, policy, M, seed=0, first_env=0):
        self.policy, self.M, self.seed, self.first_env = policy, int(M), int(seed), int(first_env)
        self.key = None
        self.decision = None  # the SampleDecision in force
        self.act = self.logp = self.feat_c = None  # the last step's records

    def _check(self, obs, what):
        if torch.is_tensor(obs) and obs.dim() == 2 and obs.shape[0] != self.M:
            raise ValueError(f"SamplingSession.{what} takes one row per stream: [{self.M}, {self.policy.obs_dim}]")

    def begin(self, obs, iteration=0, want_probs=False, want_features=False, status=None):
        self._check(obs, "begin")
        self.key = noise_key(self.seed, iteration)
        self.decision = self.policy.sample_decide(obs, key=self.key, first_env=self.first_env, want_probs=want_probs,
                                                  want_features=want_features, status=status)
        return self.decision

    def step(self, obs, t, status=None):
        self._check(obs, "step")
        if self.decision is None:
            raise ValueError("SamplingSession.step before begin")
        d = self.decision
        r = self.policy.sample_act(obs, d.a_d, d.closest, key=self.key, first_env=self.first_env, t=t, status=status)
        self.act, self.logp, self.feat_c = r.act, r.logp, r.feat_c
        return r.actions
