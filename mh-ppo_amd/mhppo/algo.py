"""Env_rollout / Algo_PPO with the reference's API, running on the MI355X path.

Drop-in surface of Coop-MH-PPO-scalable.py §3-§4 (:96-1001) and the coop
driver (Coop-MH-PPO.ipynb cell 0): same class names, constructor arguments,
method names, hyper-parameter defaults and checkpoint file names/keys.  The
environment is a VecCrosswalk of N envs: one `train` iteration plays one
80-step episode in every env (the reference plays 26 episodes of one env for
batch_size=2048), then runs the same 10 + 10 full-batch epochs.
"""
import contextlib
import os

import numpy as np
import torch
import torch.distributed as dist

from . import _lib, ppo, shuffle
from .env import VecCrosswalk
from .models import Model_PPO
from .rollout import RolloutGPU, bucket_segments

PREFIX = {"scalable": "pappo-scalable-coop", "coop": "pappo-coop", "4cars": "pappo-coop-4cars", "naif": "pappo-acc6"}


def _rank():
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _rank_path(path):
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return f"{path}.rank{dist.get_rank()}"
    return path


def _venv(env):
    return env.venv if hasattr(env, "venv") else env


# The asynchronous read-backs of train() (reward-curve sums, diagnostics sums, gradient norms): an
# iteration queues (host copy, event, *payload) without a host sync, and the entry is appended to
# its list once the copy has landed, one iteration later or when curves() / the end of train() asks.
def _readback(t, *payload):
    """Queue entry for device tensor `t`: on the GPU a non-blocking copy to pinned memory and an
    event on the current stream; on the CPU (test doubles: tests/test_dp_gloo.py) a clone, no event."""
    if t.device.type == "cuda":
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        host.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(t.device))
    else:
        host, ev = t.clone(), None
    return (host, ev, *payload)


def _land(queue, append, keep_last=False):
    """append(host, *payload) for every entry of `queue` (keep_last: all but the newest, whose copy
    may still be in flight), waiting for its event; the entries leave the queue."""
    n = len(queue) - (1 if keep_last else 0)
    for host, ev, *payload in queue[:n]:
        if ev is not None:
            ev.synchronize()
        append(host, *payload)
    del queue[:n]


class Env_rollout:
    """Batched Env_rollout (:96-684): collects one episode per env per call."""

    def __init__(self, env, nb_cars, max_steps, dt):
        self.env = _venv(env)
        self.nb_cars = nb_cars
        self.dt = dt
        self.max_steps = max_steps
        self.shape_env = 2 + 9 + 2
        self.gpu = RolloutGPU(self.env, T=max_steps)
        self.shape_env_d = self.gpu.dc
        self.seed = 0
        self.iteration = 0
        self.fix_bucket = False  # opt-in bug fix (Algo_PPO.fix_bucket)
        # opt-in GAE(lambda) targets (Algo_PPO.gae_lambda): (critic_cross, critic_wait, gamma, lam)
        self.gae = None
        self.env.reset(want_obs=False)  # the reference's __init__ resets the env (:107)
        self.batch = None
        self.cross = self.wait = self.choice = None

    def reset(self):
        """(:125-144) clears the batches and resets the env, consuming that reset's draws
        in every env's random stream exactly as the reference does."""
        self.env.reset(want_obs=False)
        self.batch = None
        self.cross = self.wait = self.choice = None

    def iterations(self, actor_net_cross, actor_net_wait, actor_net_choice, nbr_episodes, choix=False):
        """Deterministic evaluation (:152-252) of `nbr_episodes` consecutive episodes in every
        env; returns (obs, acts, rews_c, rews_d, waiting_time) env-major (see RolloutGPU.evaluate).
        choix=True: the scripted choix_test scenario (:629-633) after every reset."""
        with torch.no_grad():
            return self.gpu.evaluate(actor_net_cross, actor_net_wait, actor_net_choice, nbr_episodes, choix=choix)

    def iterations_stats(self, actor_net_cross, actor_net_wait, actor_net_choice, nbr_episodes, choix=False):
        """iterations() reduced on the device to get_average's sums (RolloutGPU.evaluate_stats;
        opt-in, beyond the reference): float64 [MHPPO_EVS_N] on the env's device, no trajectory."""
        with torch.no_grad():
            return self.gpu.evaluate_stats(actor_net_cross, actor_net_wait, actor_net_choice, nbr_episodes,
                                           choix=choix)

    def iterations_rand(self, actor_net_cross, actor_net_wait, actor_net_choice, cov_mat=None, cov_mat_d=None,
                        batch_size=None, random_rate=0.0, forced_choice=None, eps_tape=None):
        """One episode in every env (:357-517); buckets the segments like :489-507."""
        with torch.no_grad():
            self.batch = self.gpu.collect(actor_net_cross, actor_net_wait, actor_net_choice, seed=self.seed,
                                          iteration=self.iteration, forced_choice=forced_choice, eps_tape=eps_tape)
        self.iteration += 1
        # NaN policy outputs raise, as torch.distributions does in the reference: the status word
        # comes back with the bucket sizes (the iteration's one host sync before the update)
        self.cross, self.wait, self.choice = bucket_segments(self.batch, fix_bucket=self.fix_bucket,
                                                             status=self.gpu.status, gae=self.gae)
        return self.batch

    # reference-named views of the collected batch
    @property
    def batch_obs_cross(self):
        return self.cross["obs"]

    @property
    def batch_obs_wait(self):
        return self.wait["obs"]

    @property
    def batch_obs_choice(self):
        return self.choice["obs"]

    def futur_rewards(self):
        """(:658-684) reward-to-go per bucket (float32); choice = episodic min."""
        return self.cross["ret"], self.wait["ret"], self.choice["ret"]

    def immediate_rewards(self):
        """(:635-656)"""
        return self.cross["rew"].float(), self.wait["rew"].float(), self.choice["ret"]


class Algo_PPO:
    """Multi-head PPO (:698-1001)."""

    def __init__(self, policy_class, env, **hyperparameters):
        self._init_hyperparameters(hyperparameters)
        venv = _venv(env)
        self.venv = venv
        self.max_steps = venv.max_episode
        S = venv.n_slots
        if not hasattr(self, "num_states_c"):
            self.num_states_c = 13
        if not hasattr(self, "num_states_d"):
            self.num_states_d = _lib.lib().mhppo_choice_dim(venv.handle)
        if not hasattr(self, "num_actions"):
            self.num_actions = 1
        if not hasattr(self, "mean"):
            self.mean = (venv.cfg.car_b[2] + venv.cfg.car_b[0]) / 2.0   # :1044
        if not hasattr(self, "std"):
            self.std = (venv.cfg.car_b[2] - venv.cfg.car_b[0]) / 2.0    # :1045
        if not hasattr(self, "dt"):
            self.dt = venv.dt
        dev = venv.device
        self.actor_net_cross = policy_class(self.num_states_c, self.num_actions, 1, nb_car=S, mean=self.mean,
                                            std=self.std).to(dev)
        self.actor_net_wait = policy_class(self.num_states_c, self.num_actions, 1, nb_car=S, mean=self.mean,
                                           std=self.std).to(dev)
        self.actor_net_choice = policy_class(self.num_states_d, 2, 2).to(dev)
        self.critic_net_cross = policy_class(self.num_states_c, 1, 0).to(dev)
        self.critic_net_wait = policy_class(self.num_states_c, 1, 0).to(dev)
        self.critic_net_choice = policy_class(self.num_states_d, 1, 0).to(dev)
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            for net in self.nets():  # replicas start identical (rank 0's init)
                for p in net.parameters():
                    dist.broadcast(p.data, src=0)
        # every net's flat gradient in one contiguous buffer: one in-place all-reduce per
        # joint epoch under data parallelism (mhppo.ppo.GradBucket)
        # (actors first, then critics: the first and last steps of the epoch pipeline, which train
        # only the critics / only the actors, reduce one contiguous span too)
        self.grad_bucket = ppo.GradBucket([self.actor_net_cross, self.actor_net_wait, self.actor_net_choice,
                                           self.critic_net_cross, self.critic_net_wait, self.critic_net_choice],
                                          dev)
        # one fused Adam launch per net and step on the GPU (the reference's default Adam
        # semantics: lr, betas (0.9, 0.999), eps 1e-8, no weight decay)
        A = (lambda params, lr: torch.optim.Adam(params, lr, fused=True)) if dev.type == "cuda" else torch.optim.Adam
        self.optimizer_critic_cross = A(self.critic_net_cross.parameters(), self.critic_lr)
        self.optimizer_critic_wait = A(self.critic_net_wait.parameters(), self.critic_lr)
        self.optimizer_critic_choice = A(self.critic_net_choice.parameters(), self.critic_d_lr)
        self.optimizer_actor_cross = A(self.actor_net_cross.parameters(), self.actor_lr)
        self.optimizer_actor_wait = A(self.actor_net_wait.parameters(), self.actor_lr)
        self.optimizer_actor_choice = A(self.actor_net_choice.parameters(), self.actor_d_lr)
        self.value_std = 0.5
        self.value_std_d = 0.1
        self.cov_var = torch.full(size=(self.num_actions,), fill_value=self.value_std)
        self.cov_mat = torch.diag(self.cov_var)
        self.cov_var_d = torch.full(size=(2 * S,), fill_value=self.value_std_d)
        self.cov_mat_d = torch.diag(self.cov_var_d)
        self.rollout = Env_rollout(venv, S, self.max_steps, self.dt)
        self.rollout.seed = getattr(self, "seed", 0)
        # reward curves (:886-892).  While train() runs with verbose=False they lag by one
        # iteration: an iteration's sums are read back asynchronously and appended at the next
        # iteration (or at the end of train()); curves() / save_checkpoint() flush them first.
        self.ep_reward_cross, self.ep_reward_wait, self.ep_reward_choice = [], [], []
        self.ep_scenario_balance = []
        self._pending_curves = []  # (pinned sums, event, m_c, m_w, m_d) not yet appended
        self.last_losses = {}
        # Opt-in per-iteration PPO diagnostics (Algo_PPO(diagnostics=True, diagnostics_every=k)):
        # after the update of every k-th iteration one forward-only launch per trained head
        # (mhppo.ppo.k_ppo_diag) over that iteration's batch with the post-update nets; the entries
        # {"iteration": i, "cross": {...}, "wait": {...}, "choice": {...}} (mhppo.ppo.diag_stats;
        # only the heads trained that iteration) land in self.diagnostics like the reward curves,
        # without a host sync in the iteration.  Not checkpointed: save_checkpoint keeps the
        # reward curves only, and a resumed run starts with an empty list.
        self._diag_on = bool(self.diagnostics)
        self.diagnostics = []
        self._pending_diag = []   # (pinned [H, DIAG_N] sums, event, iteration, [(name, m, kind)])
        self._diag_heads = None   # update()'s (name, Head) list of the current iteration
        self._diag_work = {}      # per head name: the launch's scratch, allocated once
        # Opt-in gradient norms (Algo_PPO(max_grad_norm=c)): one entry per iteration,
        # {"iteration": i, "actor_cross": [10 norms], "critic_cross": [...], ...}: per net trained
        # that iteration the float64 norm of its (all-reduced) gradient BEFORE clipping at each of
        # its 10 Adam steps.  They land like the reward curves (asynchronous copy, appended one
        # iteration later, flushed by curves()).  Not checkpointed: a resumed run starts empty.
        self.grad_norms = []
        self._pending_norms = []  # (pinned [10, 2H] norms, event, iteration, head names)
        self._norms_dev = None    # update()'s (norms tensor, head names) of the current iteration
        # Opt-in KL early stop (Algo_PPO(target_kl=tau)): one entry per iteration,
        # {"iteration": i, "cross": {"actor_steps": s, "approx_kl": [KL_1 .. KL_9]}, ...} for the heads
        # trained that iteration: s the actor's Adam steps (10 when it never stopped), KL_e the
        # approximate KL of the actor after e steps (after a stop the values repeat).  They land like
        # the gradient norms.  Not checkpointed: a resumed run starts empty.
        self.kl_stops = []
        self._pending_kl = []     # (pinned [9 H 2 + H] doubles, event, iteration, head names, row counts)
        self._kl_dev = None       # update()'s (kl, stop, head names, row counts) of the current iteration
        self._external = None    # train_external's (its arguments' key, ExternalRollout): its buffers are allocated once

    def nets(self):
        return [self.actor_net_cross, self.actor_net_wait, self.actor_net_choice, self.critic_net_cross,
                self.critic_net_wait, self.critic_net_choice]

    def _init_hyperparameters(self, hyperparameters):
        """(:919-933) defaults; overrides set as attributes (the reference uses exec)."""
        self.num_algo = 1
        self.total_loop = 0
        self.batch_size = 2048
        self.gamma = 0.99
        self.critic_lr = 1e-3
        self.actor_lr = 3e-4
        self.critic_d_lr = 1e-3
        self.actor_d_lr = 3e-4
        self.verbose = True
        # opt-in bug fixes, off for parity: bucket cars by their closest
        # pedestrian's decision; per-row choice loss (not the M x M broadcast).  The scalable
        # lane fix is an env option: VecCrosswalk(..., fix_scalable_lanes=True).
        self.fix_bucket = False
        self.fix_choice_loss = False
        # all heads trained on the exact f32-MFMA kernel (k-ordered fmaf sums) instead of the
        # default bf16x3 split-precision one (f32-level products at 2.67x the f32-MFMA ceiling)
        self.exact_f32 = False
        # reward curves written to load_model/parameters at the end of train() (:908-916)
        self.save_curves = True
        # per-iteration diagnostics (approximate KL, clip fraction, entropy, explained variance),
        # every diagnostics_every-th iteration; off: the iteration runs exactly the code it always did
        self.diagnostics = False
        self.diagnostics_every = 1
        # GAE(lambda) targets for the cross and wait heads (beyond the reference, which trains on the
        # Monte-Carlo reward-to-go): None = off, the iteration runs exactly the code it always did;
        # a value in [0, 1] makes the buckets' `ret` the lambda-returns A_t + V_old(s_t) under the
        # pre-update critics (mhppo.rollout.gae_targets_tm), so the train kernels' A = ret - V is the
        # GAE advantage in epoch 0 and the critics regress on the lambda-returns.  1.0 is the
        # reward-to-go again (to float64 rounding).  The choice head keeps its episodic-min target.
        # Nothing of it is checkpointed; the diagnostics' explained variance and value MSE are then
        # relative to the lambda-returns (they read the buckets' `ret`).
        self.gae_lambda = None
        # gradient-norm clipping (beyond the reference, whose steps are unbounded): None = off, the
        # iteration runs exactly the code it always did; a float > 0 clips every net's gradient to
        # that norm before each of its Adam steps, the first included, on the native clip-and-Adam
        # launch (mhppo.adam.adam_clip_steps); inf clips nothing and only records the norms
        # (self.grad_norms).  A constructor argument, as gae_lambda is: nothing of it is checkpointed.
        self.max_grad_norm = None
        # minibatch updates (beyond the reference, whose ten epochs per head are full-batch): None =
        # off, update() makes exactly the calls it always did; an integer K >= 1 runs every epoch as K
        # minibatch steps per head on a fresh keyed shuffle of the head's batch
        # (mhppo.ppo.train_minibatches: each step is train_epoch on a slice, so every optimiser takes
        # 10 K steps per iteration and the advantage is normalised per minibatch).  The shuffle's key
        # is mhppo.shuffle.shuffle_key(rollout.seed, the iteration the batch was collected in, epoch,
        # head index, the shard's first global env id): no generator state, so nothing of it is
        # checkpointed and a resumed run draws the same minibatches.  A constructor argument, as
        # gae_lambda is.  Under data parallelism every rank shuffles its own shard: a different draw
        # of minibatches than one process on all envs.
        self.minibatches = None
        # KL early stopping (beyond the reference, whose ten epochs per head are unconditional; the
        # target_kl of Spinning Up, SB3, CleanRL and RLlib): None = off, update() makes exactly the
        # calls it always did; a float tau > 0 measures, before each actor step but the first, the
        # approximate KL of the head's current policy from the one that collected the batch
        # (mhppo.ppo.k_ppo_kl: the diagnostics' approx_kl over the whole batch) and stops that head's
        # ACTOR for the rest of the iteration once it exceeds 1.5 tau; the critic takes all ten steps
        # (Spinning Up's rule).  The decision is made on the device inside the clip-and-Adam launch
        # (mhppo.ppo.train_epochs): no host sync, and every step of the iteration then runs on the
        # native launch, as with max_grad_norm.  A stopped actor's train passes still run (their
        # gradient is discarded).  inf never stops and only records (self.kl_stops).  Not with
        # minibatches.  A constructor argument, as gae_lambda is: nothing of it is checkpointed.
        self.target_kl = None
        for k, v in hyperparameters.items():
            setattr(self, k, v)
        if self.target_kl is not None:
            tau = float(self.target_kl)
            if not tau > 0.0:  # (NaN fails the comparison)
                raise ValueError(f"target_kl must be None or a float > 0 (inf allowed), not {self.target_kl!r}")
            if self.minibatches is not None:
                raise ValueError("target_kl does not combine with minibatches: the gate is per full-batch epoch")
            self.target_kl = tau
        if self.max_grad_norm is not None:
            c = float(self.max_grad_norm)
            if not c > 0.0:  # (NaN fails the comparison)
                raise ValueError(f"max_grad_norm must be None or a float > 0 (inf allowed), not {self.max_grad_norm!r}")
            self.max_grad_norm = c
        if self.gae_lambda is not None:
            lam = float(self.gae_lambda)
            if not 0.0 <= lam <= 1.0:  # (NaN fails both comparisons)
                raise ValueError(f"gae_lambda must be None or in [0, 1], not {self.gae_lambda!r}")
            if not 0.0 <= float(self.gamma) <= 1.0:
                raise ValueError(f"gae_lambda needs gamma in [0, 1], not {self.gamma!r}")
            self.gae_lambda = lam
        if self.minibatches is not None:
            k = self.minibatches
            if isinstance(k, bool) or not isinstance(k, int) or k < 1:
                raise ValueError(f"minibatches must be None or an integer >= 1, not {k!r}")

    def update(self):
        """10 epochs of cross+wait, then 10 epochs of choice (:868-882) on the collected batch,
        run as 10 joint epochs of the three independent heads in one pipeline of 11 steps
        (mhppo.ppo.train_epochs: same results, two collectives per step under data parallelism).
        The global row counts and choice action counts take one all-reduce and one host sync per
        iteration.  With minibatches=K the ten epochs run as 10 K minibatch steps instead
        (mhppo.ppo.train_minibatches); the heads' global slice sizes travel in the same all-reduce."""
        r = self.rollout
        dev = self.venv.device
        c, w, d = r.cross, r.wait, r.choice
        K = getattr(self, "minibatches", None)
        with (torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()):
            counts = d.get("counts")  # queued with the bucketing, before its host sync
            if counts is None:
                counts = torch.stack([(d["act"] == 0).sum(), (d["act"] == 1).sum()]).to(torch.float64)
            if ppo._dp():  # global row counts: one all-reduce and one host sync
                rows = [c["ret"].numel(), w["ret"].numel(), d["ret"].numel()]
                if K is not None:  # followed by the three heads' local slice sizes, [3, K]
                    for n in rows[:3]:
                        b = shuffle.slice_bounds(n, K)
                        rows += [b[j + 1] - b[j] for j in range(K)]
                loc = torch.cat([torch.tensor(rows, dtype=torch.float64, device=dev), counts])
                ppo._allreduce_(loc)
                n = len(rows)
                slice_m = None
                if K is None:
                    m_c, m_w, m_d = loc[:3].tolist()
                else:
                    host = loc[:n].tolist()
                    m_c, m_w, m_d = host[:3]
                    slice_m = {k: host[3 + i * K:3 + (i + 1) * K] for i, k in enumerate(("cross", "wait", "choice"))}
                counts = loc[n:n + 2]
            else:  # the local counts are the global ones, known on the host: no sync
                m_c, m_w, m_d = float(c["ret"].numel()), float(w["ret"].numel()), float(d["ret"].numel())
                slice_m = None  # the local slice sizes are the global ones: train_minibatches forms them
            heads, names = [], []
            # the reference trains a continuous head only on a non-empty batch (:869, :874); its choice
            # batch is never empty (>= 1 existing car per episode; it would raise there)
            for name, kind, b, m in (("cross", "c", c, m_c), ("wait", "c", w, m_w), ("choice", "d", d, m_d)):
                if m > 0:
                    heads.append(ppo.Head(kind, getattr(self, f"actor_net_{name}"), getattr(self, f"critic_net_{name}"),
                                          getattr(self, f"optimizer_actor_{name}"),
                                          getattr(self, f"optimizer_critic_{name}"), b["obs"], b["act"], b["logp"],
                                          b["ret"], m, counts if kind == "d" else None,
                                          per_row=kind == "d" and self.fix_choice_loss, exact=self.exact_f32))
                    names.append(name)
            clip = getattr(self, "max_grad_norm", None)
            tau = getattr(self, "target_kl", None)
            if K is not None:
                losses = self._update_minibatches(heads, names, K, clip, slice_m) if heads else None
            elif tau is not None:
                losses = None
                if heads:
                    losses, norms, kl, stop = ppo.train_epochs(heads, 10, self.grad_bucket, clip, tau)
                    self._norms_dev = None if norms is None else (norms, names)
                    self._kl_dev = (kl, stop, names, [h.m for h in heads])
            elif clip is None:
                losses = ppo.train_epochs(heads, 10, self.grad_bucket) if heads else None
            else:
                losses, norms = ppo.train_epochs(heads, 10, self.grad_bucket, clip) if heads else (None, None)
                self._norms_dev = None if norms is None else (norms, names)
            if getattr(self, "_diag_on", False):
                self._diag_heads = list(zip(names, heads))
        if self.verbose and losses is not None:
            div = {"cross": (m_c, m_c), "wait": (m_w, m_w), "choice": (m_d * m_d, m_d)}
            if self.fix_choice_loss:
                div["choice"] = (m_d, m_d)
            if K is not None:
                # the losses of each head's last minibatch step, over that step's m (a head in
                # `heads` has rows, so it is trained in at least one step)
                div = {k: ((m * m if k == "choice" and not self.fix_choice_loss else m), m)
                       for k, (_, _, m) in zip(names, losses)}
            self.last_losses = {k: (float(x[0].item()) / div[k][0], float(x[1].item()) / div[k][1])
                                for k, x in zip(names, losses)}
        return m_c, m_w, m_d

    def _update_minibatches(self, heads, names, K, clip, slice_m):
        """update() with minibatches=K: mhppo.ppo.train_minibatches over the iteration's heads, the
        shuffle keyed by mhppo.shuffle.shuffle_key (the batch was collected in iteration
        rollout.iteration - 1: iterations_rand has counted it already)."""
        r, v = self.rollout, self.venv
        env0 = int(getattr(v, "env_id_offset", getattr(getattr(v, "cfg", None), "env_id_offset", 0)))
        seed, it = int(r.seed), int(r.iteration) - 1
        idx = [shuffle.HEAD_INDEX[n] for n in names]
        res = ppo.train_minibatches(heads, 10, K, lambda e, i: shuffle.shuffle_key(seed, it, e, idx[i], env0),
                                    self.grad_bucket, clip, None if slice_m is None else [slice_m[n] for n in names])
        if clip is None:
            return res
        self._norms_dev = (res[1], names)
        return res[0]

    def evaluate(self, nbr_episodes, choix=False):
        """(:738-747) rollout.reset() then the deterministic iterations; with N envs every env
        plays `nbr_episodes` episodes (N * nbr_episodes in total, env-major)."""
        self.rollout.reset()
        return self.rollout.iterations(self.actor_net_cross, self.actor_net_wait, self.actor_net_choice,
                                       nbr_episodes, choix=choix)

    def evaluate_stats(self, nbr_episodes, choix=False):
        """get_average(evaluate(nbr_episodes)[0]) without the trajectories (opt-in, beyond the
        reference): the same reset, episodes and env draws as evaluate(), reduced on the device to
        the statistics' sums (memory O(N) whatever nbr_episodes is), all-reduced once under data
        parallelism, then mhppo.stats.stats_from_sums.  Same keys as get_average; float64 sums
        where get_average reduces in float32.  Episodes are the true ones (N * nbr_episodes): under
        choix=True, where every episode has crosswalk width 3, get_average sees one long run instead."""
        from .stats import check_variant, stats_from_sums
        check_variant(self.venv.variant)
        self.rollout.reset()
        sums = self.rollout.iterations_stats(self.actor_net_cross, self.actor_net_wait, self.actor_net_choice,
                                             nbr_episodes, choix=choix)
        ppo._allreduce_(sums)
        return stats_from_sums(sums, self.venv.nb_car)

    def policy(self):
        """The deterministic policy of evaluate() as a function of observation rows (mhppo.policy
        .Policy; opt-in, beyond the reference) on the live actors: it reads their weights at every
        call, so it tracks training."""
        from .policy import Policy
        return Policy.from_env(self.venv, self.actor_net_cross, self.actor_net_wait, self.actor_net_choice)

    def get_average(self, states):
        """The paper cell's evaluation statistics (get_average, :1550-1675; CO2 leg excluded)
        over `states`, the observations evaluate() returned (mhppo.stats)."""
        from .stats import get_average
        v = self.venv
        return get_average(states, v.variant, v.nb_car, v.nb_ped, v.nb_lines)

    def train(self, nb_loop, replay=None):
        """(:854-917): per iteration rollout.reset() -> one episode per env -> 10 + 10 epochs
        -> reward curves -> rollout.reset() (both resets consume env draws, as in the
        reference); at the end the curves go to load_model/parameters/*.npy (:908-916).
        replay (parity tests): one (forced_choice, eps_tape) pair per iteration, the
        recorded Categorical and MVN draws replayed instead of Philox noise."""
        self.rollout.fix_bucket = self.fix_bucket
        lam = getattr(self, "gae_lambda", None)
        # the critics are read when the buckets are built, before the iteration's update
        self.rollout.gae = None if lam is None else (self.critic_net_cross, self.critic_net_wait, self.gamma, lam)
        for ep in range(nb_loop):
            self.rollout.reset()
            fc, et = replay[ep] if replay is not None else (None, None)
            self.rollout.iterations_rand(self.actor_net_cross, self.actor_net_wait, self.actor_net_choice,
                                         self.cov_mat, self.cov_mat_d, self.batch_size, forced_choice=fc,
                                         eps_tape=et)
            self._after_collect(ep)
        self._finish_train()

    def train_external(self, sim, nb_loop, M, T=None, early_end=None, check_every=None, bootstrap=False,
                       cut_truncates=True, auto_reset=None):
        """train() with the rollout replaced (opt-in, beyond the reference): every iteration plays one
        episode of M parallel streams in `sim` -- anything with reset() -> obs float32 [M, obs_dim] and
        step(actions float64 [M, 2S]) -> (obs, rew, rew_light, ...) on this algo's device -- through
        mhppo.external.ExternalRollout on self.policy(), with the collector's noise of (rollout.seed,
        rollout.iteration) and the env's env_id_offset as the first global env id; then the bucketing
        and everything train() does from update() on.  The algo's own env is the config carrier only
        (it may have n_envs = 1) and is not touched: no rollout.reset().  Episodes have the fixed length
        T (default: the env's max_episode) and the simulator's done is ignored, unless early_end=True:
        then step's fourth value is the per-stream done, the step that first reports it is the stream's
        last and terminal, and the buckets are ragged (ExternalRollout(early_end=True); check_every=n
        lets the host stop an episode once every stream has ended, at one read every n steps).
        bootstrap=True (needs early_end=True): step's fifth value is the per-stream truncated, and an
        episode that was truncated -- at a done flagged so, or still running at the T-step cut unless
        cut_truncates=False -- starts its cross / wait targets from V(s_L) under the current critics
        instead of 0 (ExternalRollout(bootstrap=True), bucket_segments(boot=...)).
        auto_reset=E (an integer >= 1; needs no early_end=True, and early_end=False with it raises): the
        simulator resets a stream the moment it reports done, and every stream plays up to E episodes
        inside the T-step window, each with its own choice decision, bucket and targets
        (ExternalRollout(auto_reset=E)); step returns no truncated, and with bootstrap=True only the
        episodes cut at the window's end are bootstrapped.  Out of scope, each a ValueError: gae_lambda
        together with auto_reset, a mid-window truncated flag, next-step auto-reset simulators, a per-slot
        done and the compact record layout.  Under data parallelism every rank feeds its own simulator
        shard."""
        from .external import ExternalRollout
        r = self.rollout
        r.fix_bucket = self.fix_bucket
        lam = getattr(self, "gae_lambda", None)
        r.gae = None if lam is None else (self.critic_net_cross, self.critic_net_wait, self.gamma, lam)
        if auto_reset is not None:
            # checked before it goes into the cache key: True, 1 and 1.0 hash alike
            if isinstance(auto_reset, bool) or not isinstance(auto_reset, int) or auto_reset < 1:
                raise ValueError(f"train_external: auto_reset is None or an integer >= 1, not {auto_reset!r}")
            if early_end is not None and not early_end:
                raise ValueError("train_external: auto_reset implies early_end: early_end=False with it is a contradiction")
            if lam is not None:
                raise ValueError("train_external: gae_lambda together with auto_reset is out of scope (the "
                                 "lambda-return kernel takes one length per column)")
            early_end = True
        if bootstrap and not early_end:
            raise ValueError("train_external: bootstrap=True needs early_end=True")
        # cut_truncates means nothing without bootstrap, auto_reset nothing when unset: the key is then the one it was
        key = (int(M), int(T or self.max_steps), bool(early_end)) + ((True, bool(cut_truncates)) if bootstrap else ())
        key += () if auto_reset is None else (("auto_reset", auto_reset),)
        if getattr(self, "_external", None) is None or self._external[0] != key:
            self._external = (key, ExternalRollout(self.policy(), key[0], T=key[1], early_end=key[2],
                                                   bootstrap=bool(bootstrap), cut_truncates=bool(cut_truncates),
                                                   auto_reset=auto_reset))
        # the critics are read when the buckets are built, before the iteration's update
        boot = (self.critic_net_cross, self.critic_net_wait) if bootstrap else None
        ext = self._external[1]
        ext.session.first_env = int(self.venv.cfg.env_id_offset)
        for ep in range(nb_loop):
            ext.session.seed = int(r.seed)
            r.batch = ext.collect(sim, r.iteration, check_every=check_every)
            r.iteration += 1
            r.cross, r.wait, r.choice = bucket_segments(r.batch, fix_bucket=r.fix_bucket, status=ext.status,
                                                        gae=r.gae, boot=boot)
            self._after_collect(ep, reset_env=False)
        self._finish_train()

    def _after_collect(self, ep, reset_env=True):
        """The rest of an iteration once rollout.cross / wait / choice hold its batch: the update, the
        queued diagnostics, gradient norms and reward-curve read-back, the closing rollout.reset()
        (train(); train_external leaves the algo's own env alone), total_loop, and landing the previous
        iteration's entries."""
        m_c, m_w, m_d = self.update()
        dev = self.venv.device
        diag = getattr(self, "_diag_on", False)
        if diag and self.total_loop % max(1, int(self.diagnostics_every)) == 0:
            self._queue_diagnostics()
        if getattr(self, "_norms_dev", None) is not None:
            self._queue_grad_norms()
        if getattr(self, "_kl_dev", None) is not None:
            self._queue_kl_stops()
        # the reward curves' sums over (cross, wait, choice): from the bucketing pass on the GPU
        # (bucket_segments: fixed-order float64 partials), else torch reductions
        sums = (self.rollout.choice or {}).get("rew_sums")
        if sums is None:
            rc, rw, rd = self.rollout.immediate_rewards()
            sums = torch.stack([rc.double().sum(), rw.double().sum(), rd.double().sum()]).to(dev)
        elif ppo._dp():
            sums = sums.clone()  # the all-reduce below is in place
        ppo._allreduce_(sums)
        # the reward curves take the sums without a host sync here
        self._pending_curves.append(_readback(sums, m_c, m_w, m_d))
        if self.verbose:
            self._flush_curves()
        if self.verbose and _rank() == 0:
            print("Episode * {} * And Number of steps is ==> {}".format(ep, ep * self.batch_size))
            print("Average Cross reward is ==> {}, Average Wait reward is ==> {}".format(
                np.mean(self.ep_reward_cross[-10:]) if self.ep_reward_cross else float("nan"),
                np.mean(self.ep_reward_wait[-10:]) if self.ep_reward_wait else float("nan")))
            print("Average Choice reward is ==> {}".format(np.mean(self.ep_reward_choice[-10:])))
            print("Number Cross is ==> {} and Number Wait is ==> {} ".format(int(m_c), int(m_w)))
        if reset_env:
            self.rollout.reset()
        self.total_loop = self.total_loop + 1
        self._land_pending(keep_last=True)  # the previous iteration's copies landed long ago

    def _finish_train(self):
        """The end of train(): every pending entry lands, rank 0 saves the reward curves (:908-916)."""
        self._land_pending()
        if _rank() == 0 and self.save_curves:
            self.save_reward_curves()
        if self.verbose and _rank() == 0:
            print("Complete")

    def _land_pending(self, keep_last=False):
        """Land the queued read-backs of the reward curves, the gradient norms, the KL stops and the
        diagnostics (keep_last: all but each queue's newest entry).  A queue an object lacks is empty."""
        for name, append in (("_pending_curves", self._append_curves), ("_pending_norms", self._append_grad_norms),
                             ("_pending_kl", self._append_kl_stops), ("_pending_diag", self._append_diagnostics)):
            _land(getattr(self, name, []), append, keep_last)

    def _flush_curves(self):
        _land(self._pending_curves, self._append_curves)

    def _append_curves(self, host, m_c, m_w, m_d):
        """One iteration's reward-curve entries (rew_batch.mean() over the global batch, :886-892)
        from its read-back reward sums."""
        s = host.tolist()
        if m_c > 0:
            self.ep_reward_cross.append(s[0] / m_c)
        if m_w > 0:
            self.ep_reward_wait.append(s[1] / m_w)
        self.ep_reward_choice.append(s[2] / m_d if m_d > 0 else float("nan"))  # mean() of empty: NaN
        self.ep_scenario_balance.append([int(m_c), int(m_w)])

    def _queue_diagnostics(self):
        """One diagnostics launch per head update() just trained (post-update nets, this
        iteration's buckets), one all-reduce of the stacked sums under data parallelism, and their
        read-back (appended by _append_diagnostics once it has landed)."""
        heads = self._diag_heads or []
        if not heads:
            return
        with torch.cuda.device(self.venv.device):
            rows = []
            for name, h in heads:
                h._diag_work = self._diag_work.get(name)
                rows.append(ppo.k_ppo_diag(h))
                self._diag_work[name] = h._diag_work
            sums = torch.stack(rows)  # [H, DIAG_N]
            ppo._allreduce_(sums)
            self._pending_diag.append(_readback(sums, int(self.total_loop),
                                                [(name, h.m, h.kind) for name, h in heads]))

    def _append_diagnostics(self, host, it, heads):
        entry = {"iteration": it}
        for row, (name, m, kind) in zip(host.tolist(), heads):
            entry[name] = ppo.diag_stats(row, m, entropy=(kind == "d"))
        self.diagnostics.append(entry)

    def _queue_grad_norms(self):
        """The iteration's gradient norms (update()'s device tensor) on their way to the host,
        appended by _append_grad_norms once they have landed.  The norms are the replicated,
        all-reduced gradients': equal on every rank, no collective."""
        norms, names = self._norms_dev
        self._norms_dev = None
        self._pending_norms.append(_readback(norms, int(self.total_loop), list(names)))

    def _append_grad_norms(self, host, it, names):
        """One grad_norms entry (train_epochs' layout: column j head j's critic, column H + j its
        actor)."""
        cols = host.t().tolist()
        H = len(names)
        entry = {"iteration": it}
        for kind, off in (("actor", H), ("critic", 0)):
            for j, name in enumerate(names):
                entry[f"{kind}_{name}"] = cols[off + j]
        self.grad_norms.append(entry)

    def _queue_kl_stops(self):
        """The iteration's KL sums and stop words (update()'s device tensors) on their way to the
        host in one copy, appended by _append_kl_stops once they have landed.  The sums are global
        and the stops replicated: equal on every rank, no collective."""
        kl, stop, names, ms = self._kl_dev
        self._kl_dev = None
        both = torch.cat([kl.reshape(-1), stop.to(torch.float64)])
        self._pending_kl.append(_readback(both, int(self.total_loop), list(names), list(ms)))

    def _append_kl_stops(self, host, it, names, ms):
        """One kl_stops entry from train_epochs' kl [E - 1, H, 2] and stop [H] (flattened, the stops last)."""
        H = len(names)
        flat = host.tolist()
        kl, stop = flat[:len(flat) - H], flat[len(flat) - H:]
        E1 = len(kl) // (2 * H)
        entry = {"iteration": it}
        for i, (name, m) in enumerate(zip(names, ms)):
            entry[name] = {"actor_steps": int(stop[i]) or E1 + 1,
                           "approx_kl": [kl[(e * H + i) * 2 + 1] / m for e in range(E1)]}
        self.kl_stops.append(entry)

    def curves(self):
        """The reward curves with every pending entry appended: (cross, wait, choice, balance).
        (Also lands every pending entry of self.diagnostics, self.grad_norms and self.kl_stops.)"""
        self._land_pending()
        return self.ep_reward_cross, self.ep_reward_wait, self.ep_reward_choice, self.ep_scenario_balance

    def _curve_path(self, name):
        pre = PREFIX.get(self.venv.variant, "pappo")
        return "load_model/parameters/{}-{:02d}-{}-step-{:03d}000.npy".format(pre, self.num_algo, name,
                                                                             int(self.total_loop / 1000))

    def save_reward_curves(self):
        """(:908-916) reward_cross / reward_wait / reward_choice / scenario_balance."""
        self._flush_curves()
        os.makedirs("load_model/parameters", exist_ok=True)
        for name, v in (("reward_cross", np.array(self.ep_reward_cross)), ("reward_wait", np.array(self.ep_reward_wait)),
                        ("reward_choice", np.array(self.ep_reward_choice)),
                        ("scenario_balance", np.array(self.ep_scenario_balance).reshape((-1, 2)))):
            with open(self._curve_path(name), "wb") as f:
                np.save(f, v)

    # --------------------------------------------------------------- checkpoints
    def _path(self, head, kind, num_algo, total_loop):
        pre = PREFIX.get(self.venv.variant, "pappo")
        return "load_model/weights/{}-{}-{:02d}-{}-step-{:03d}0.pth".format(pre, head, num_algo, kind,
                                                                           int(total_loop / 10))

    def loading(self, num_algo, total_loop):
        """(:935-955) torch state_dicts, loaded without executing anything from the file."""
        self.num_algo, self.total_loop = num_algo, total_loop
        for head in ("cross", "wait", "choice"):
            for kind in ("actor", "critic"):
                net = getattr(self, f"{kind}_net_{head}")
                sd = torch.load(self._path(head, kind, num_algo, total_loop), map_location=self.venv.device,
                                weights_only=True)
                net.load_state_dict(sd)

    def loading_curriculum(self, num_actor, num_algo, total_loop):
        """(:957-983) load one head's actor + critic: 0 cross, 1 wait, 2 choice."""
        self.total_loop = total_loop
        head = ("cross", "wait", "choice")[num_actor]
        for kind in ("actor", "critic"):
            net = getattr(self, f"{kind}_net_{head}")
            net.load_state_dict(torch.load(self._path(head, kind, num_algo, total_loop),
                                           map_location=self.venv.device, weights_only=True))

    # Checkpoint/resume beyond the reference: the reference keeps only
    # weights; an exact resume also needs the Adam moments, every env's state and random
    # stream, the rollout noise counter and the reward curves.
    def _optimizers(self):
        return {f"{k}_{h}": getattr(self, f"optimizer_{k}_{h}") for h in ("cross", "wait", "choice")
                for k in ("actor", "critic")}

    def save_checkpoint(self, path):
        """Everything needed to continue training bit-identically.  Under data parallelism
        every rank writes `path.rank<r>` (its env shard differs; nets/Adam are replicated).
        The opt-in diagnostics (self.diagnostics) are not part of it: the format is unchanged."""
        self._flush_curves()  # the newest iteration's curve entries may still be in flight
        ck = {
            "nets": {f"{k}_{h}": getattr(self, f"{k}_net_{h}").state_dict() for h in ("cross", "wait", "choice")
                     for k in ("actor", "critic")},
            "optim": {k: o.state_dict() for k, o in self._optimizers().items()},
            "env": self.venv.state_dict(),
            "rollout": {"iteration": int(self.rollout.iteration), "seed": int(self.rollout.seed)},
            "algo": {"num_algo": int(self.num_algo), "total_loop": int(self.total_loop)},
            "curves": {"cross": [float(x) for x in self.ep_reward_cross],
                       "wait": [float(x) for x in self.ep_reward_wait],
                       "choice": [float(x) for x in self.ep_reward_choice],
                       "balance": [[int(a), int(b)] for a, b in self.ep_scenario_balance]},
        }
        torch.save(ck, _rank_path(path))

    def load_checkpoint(self, path):
        """Inverse of save_checkpoint (weights_only load: tensors and plain containers only)."""
        ck = torch.load(_rank_path(path), map_location="cpu", weights_only=True)
        for name, sd in ck["nets"].items():
            k, h = name.split("_")
            getattr(self, f"{k}_net_{h}").load_state_dict(sd)
        for name, o in self._optimizers().items():
            o.load_state_dict(ck["optim"][name])
        self.venv.load_state_dict(ck["env"])
        self.rollout.iteration = ck["rollout"]["iteration"]
        self.rollout.seed = ck["rollout"]["seed"]
        self.num_algo, self.total_loop = ck["algo"]["num_algo"], ck["algo"]["total_loop"]
        c = ck["curves"]
        self.ep_reward_cross, self.ep_reward_wait = list(c["cross"]), list(c["wait"])
        self.ep_reward_choice, self.ep_scenario_balance = list(c["choice"]), [list(x) for x in c["balance"]]

    def saving(self):
        """(:985-1001)"""
        os.makedirs("load_model/weights", exist_ok=True)
        for head in ("cross", "wait", "choice"):
            for kind in ("actor", "critic"):
                net = getattr(self, f"{kind}_net_{head}")
                torch.save(net.state_dict(), self._path(head, kind, self.num_algo, self.total_loop))
