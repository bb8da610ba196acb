"""Stateless policy inference: hybrid actions from observation rows, without an env.

`Policy` applies the three trained heads to float32 observation rows from anywhere (another
simulator, a recorded trajectory, a grid of observations for a decision map) on the native path
(mhppo_policy_decide / mhppo_policy_act, include/mhppo.h): the deterministic rule of the evaluation
(Env_rollout.iterations, Coop-MH-PPO-scalable.py:152-252), bit for bit what mhppo_eval_step hands
its env step.  `PolicySession` adds the evaluation's decision schedule for parallel streams of
observations.  There is no CPU path.
"""
import ctypes

import torch

from . import _lib
from .env import CAR_B, VARIANTS, _flat

MAX_P = 32  # mhppo_policy_act: a slot's pedestrians share one 32-row tile


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
