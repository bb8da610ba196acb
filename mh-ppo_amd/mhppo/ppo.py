"""PPO update of the multi-head actor-critic (Algo_PPO.train_model_c / _d,
Coop-MH-PPO-scalable.py:778-851), full batch, on the GPU.

Every head's epoch runs on the fused training kernel (mhppo_mlp_train, csrc/mlp_train.hip;
the 13-input heads on its bf16x3 split-precision MFMA path — six bf16 products per f32
product, f32-level accuracy — or, with Algo_PPO(exact_f32=True) (MHPPO_TRAIN_EXACT_F32), on f32
MFMA with k-ordered sums; the choice head on f32 MFMA): a critic pass (forward, MSE gradient, advantage sums) and an
actor pass (forward, clip-surrogate gradient against the advantage normalised with
the start-of-epoch critic, backward, weight gradients); Adam (fused) steps each net.
Epoch semantics follow the reference: the advantage uses the critic of the start of
the epoch (:784-787), the actor-loss gradient never reaches the critic (the reference
zeroes it before the critic step, :810-815).  The small HIP kernels below (advantage
statistics, the clip surrogates, MSE) restate the same losses for the tests'
autograd cross-checks.

Heads are independent nets, so one epoch of every head of an iteration runs together
(train_epoch): the reference's 10 cross/wait epochs and its 10 choice epochs
(:868-882) become 10 joint epochs with identical results.

Data parallel: every rank holds a shard of every head's batch.  Per
joint epoch there are exactly two collectives: one all-reduce (SUM, float64) of all
heads' advantage sums between the critic and the actor passes, and one all-reduce
(SUM) of the gradient bucket — every net's flat gradient lives in one contiguous
GradBucket, so the collective runs in place with no pack/unpack copies.  Each rank's
gradient is that of (global-mean loss restricted to its rows), so the reduced
gradient is the full-batch gradient; Adam then runs replicated.  A rank whose shard
of a head is empty still joins both collectives (the kernel writes a zero gradient).
"""
import contextlib
import ctypes
import math
import os

import torch
import torch.distributed as dist

from . import _lib
from .adam import (adam_clip_steps, adam_clip_sumsq, adam_clip_torch, adam_steps, clip_forget, fold_1024_4,  # noqa: F401
                   clip_prepare, gate_table)


_FORCE_COLLECTIVES = False


def set_force_collectives(flag=True):
    """Run the data-parallel collectives even in a one-rank process group (they are skipped
    when world_size == 1): a one-GPU RCCL rehearsal of the exact multi-GPU call sequence
    (bench.py --force-collectives, tests/dp_worker.py --nccl-world1).  Needs an initialised
    process group; a one-rank SUM is the identity, so results equal the plain run's."""
    global _FORCE_COLLECTIVES
    _FORCE_COLLECTIVES = bool(flag)


def _dp():
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return _FORCE_COLLECTIVES or dist.get_world_size() > 1


def _allreduce_(t):
    if _dp():
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


def global_counts(values, device):
    """All-reduce (SUM) a few per-rank counts at once; one host sync: returns floats."""
    t = torch.tensor([float(v) for v in values], dtype=torch.float64, device=device)
    return [float(x) for x in _allreduce_(t).tolist()]


def global_count(n, device):
    return global_counts([n], device)[0]


class GradBucket:
    """One contiguous float32 buffer holding the flat gradients of several Model_PPOs
    (each net's .grad views alias its slice): the gradient all-reduce of an epoch is
    one in-place collective over a contiguous span of it."""

    def __init__(self, nets, device):
        sizes = [n.flat().numel() for n in nets]
        self.buf = torch.zeros(sum(sizes), dtype=torch.float32, device=device)
        self.span = {}
        off = 0
        for net, n in zip(nets, sizes):
            net.bind_grad(self.buf[off:off + n])
            self.span[id(net)] = (off, off + n)
            off += n

    def runs(self, nets):
        """The maximal contiguous spans of the bucket covered by `nets`' gradients, in order (a
        net that is not trained this epoch — an empty head — splits the span: its stale slice is
        never reduced)."""
        spans = sorted(self.span[id(n)] for n in nets)
        out = []
        for lo, hi in spans:
            if out and out[-1][1] == lo:
                out[-1][1] = hi
            else:
                out.append([lo, hi])
        return [tuple(r) for r in out]

    def allreduce(self, nets):
        """In-place SUM of `nets`' gradients: one collective per maximal contiguous run (one for
        the usual all-heads epoch)."""
        if not _dp() or not nets:
            return
        for n in nets:  # re-link any .grad that autograd / zero_grad rebound
            n.grad_flat()
        for lo, hi in self.runs(nets):
            dist.all_reduce(self.buf[lo:hi], op=dist.ReduceOp.SUM)


def _allreduce_net_grads(*nets):
    """Gradient all-reduce for nets outside a GradBucket (one packed collective)."""
    if not _dp():
        return
    flats = [n.grad_flat() for n in nets]
    flat = torch.cat(flats)
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    off = 0
    for f in flats:
        f.copy_(flat[off:off + f.numel()])
        off += f.numel()


# ---------------------------------------------------------------- kernel layer
# Thin wrappers over the HIP entry points (include/mhppo.h).  Each returns this
# rank's LOCAL contribution; the DP orchestration below decides what is reduced.

def k_adv_stats(ret, value):
    """(sum A, sum A^2) over local rows, float64 [2]."""
    stats = torch.zeros(2, dtype=torch.float64, device=ret.device)
    v = value.detach().contiguous()
    with torch.cuda.device(ret.device):
        _lib.check(_lib.lib().mhppo_adv_stats(_lib.ptr(ret), _lib.ptr(v), ret.numel(), _lib.ptr(stats),
                                              _lib.stream_ptr()))
    return stats


def k_adv_normalize(ret, value, stats, m_global):
    adv = torch.empty_like(ret)
    v = value.detach().contiguous()
    with torch.cuda.device(ret.device):
        _lib.check(_lib.lib().mhppo_adv_normalize(_lib.ptr(ret), _lib.ptr(v), ret.numel(), _lib.ptr(stats),
                                                  float(m_global), _lib.ptr(adv), _lib.stream_ptr()))
    return adv


def k_mse(value, ret, m_global):
    dv = torch.empty_like(ret)
    loss = torch.zeros(1, dtype=torch.float64, device=ret.device)
    v = value.detach().contiguous()
    with torch.cuda.device(ret.device):
        _lib.check(_lib.lib().mhppo_mse_fwd_bwd(_lib.ptr(v), _lib.ptr(ret), ret.numel(), 1.0 / m_global,
                                                _lib.ptr(dv), _lib.ptr(loss), _lib.stream_ptr()))
    return dv, loss


def k_ppo_cont(mu, act, logp_old, adv, m_global):
    dmu = torch.empty_like(adv)
    loss = torch.zeros(1, dtype=torch.float64, device=adv.device)
    m = mu.detach().contiguous()
    with torch.cuda.device(adv.device):
        _lib.check(_lib.lib().mhppo_ppo_cont_fwd_bwd(_lib.ptr(m), _lib.ptr(act), _lib.ptr(logp_old), _lib.ptr(adv),
                                                     adv.numel(), 1.0 / m_global, _lib.ptr(dmu), _lib.ptr(loss),
                                                     _lib.stream_ptr()))
    return dmu, loss


def k_ppo_choice(probs, logp_old, adv, counts, m_global):
    p = probs.detach().contiguous()
    dp = torch.empty_like(p)
    loss = torch.zeros(1, dtype=torch.float64, device=adv.device)
    with torch.cuda.device(adv.device):
        _lib.check(_lib.lib().mhppo_ppo_choice_fwd_bwd(_lib.ptr(p), _lib.ptr(logp_old), _lib.ptr(adv), adv.numel(),
                                                       _lib.ptr(counts), 1.0 / (m_global * m_global), _lib.ptr(dp),
                                                       _lib.ptr(loss), _lib.stream_ptr()))
    return dp, loss


# Optional launch timing (bench.py): when a list, each fused train launch appends
# (kind, n_in, rows, start_event, end_event) recorded on the launch stream.
TRAIN_EVENTS = None


def flops_per_row(n_in, n_out):
    """Algorithmic FLOPs of one row through the fused kernel: forward and
    weight gradient 2 * (32 n_in + 2048 + 2048 + 32 n_out) each, backward data without
    dX 2 * (32 n_out + 2048 + 2048).  13 -> 1: 26,432."""
    macs = 32 * n_in + 2048 + 2048 + 32 * n_out
    return 2 * macs + 2 * (32 * n_out + 4096) + 2 * macs


FLOPS_PER_ROW_CONT = flops_per_row(13, 1)
N_IN_MAX = 64  # the fused kernel's widest input (scalable 8-slot choice head: dc = 54)

KIND_CRITIC, KIND_CONT, KIND_CHOICE = 0, 1, 2
# MHPPO_TRAIN_EXACT_F32 (include/mhppo.h mhppo_mlp_train): a head's passes on the f32-MFMA
# kernel (k-ordered fmaf sums, the exact f32 arithmetic of an fmaf chain) instead of the default
# bf16x3 split-precision one; per head: Head(exact=True), set by Algo_PPO(exact_f32=True)
TRAIN_EXACT_F32 = 0x100


def n_params(n_in, n_out):
    return 32 * n_in + 32 + 64 * 32 + 64 + 32 * 64 + 32 + 32 * n_out + n_out


_MODEL_TYPE = {KIND_CRITIC: 0, KIND_CONT: 1, KIND_CHOICE: 2}  # the Model_PPO.model_type a pass kind trains


def _check_net(kind, net, pair=False):
    """The one net check of the train passes: `net` is what a pass of `kind` trains (pair: as one
    of the two 13 -> 1 nets of the fused pair launch)."""
    if pair:
        if net.model_type != _MODEL_TYPE[kind] or net.n_in != 13 or net.n_out != 1:
            raise ValueError("the fused pair launch trains a 13 -> 1 continuous actor and its 13 -> 1 critic")
    elif net.model_type != _MODEL_TYPE[kind] or net.n_in > N_IN_MAX or (kind == KIND_CONT and net.n_in != 13):
        raise ValueError(f"fused kernel kind {kind} cannot train a model_type {net.model_type} "
                         f"{net.n_in}->{net.n_out} Model_PPO")


def _obs_rows(obs):
    """The observation rows as the kernels read them: float32, contiguous, 16-byte aligned."""
    obs = obs.float().contiguous()
    return obs.clone() if obs.data_ptr() % 16 else obs


def _addr(t):
    return None if t is None else t.data_ptr()


def _ev_begin():
    if TRAIN_EVENTS is None:
        return None
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    return ev


def _ev_end(ev, kind, n_in, M):
    if ev is not None:
        ev[1].record()
        TRAIN_EVENTS.append((kind, n_in, M, ev[0], ev[1]))


# The raw launchers: the one call site of each C entry point.  Addresses (or None), sizes and the
# hipStream_t handle; the caller has made the tensors' device current and keeps them alive.  The
# launch events are recorded on the current stream, which the callers make the launch stream.
def _launch_train(kind, flags, n_in, w, obs, M, ret, V, act, lp, stats, counts, m, mean, std, grad, sums, st):
    ev = _ev_begin()
    _lib.check(_lib.lib().mhppo_mlp_train(kind | flags, n_in, w, obs, M, ret, V, act, lp, stats, counts, m, mean, std,
                                          grad, sums, st))
    _ev_end(ev, kind, n_in, M)


def _launch_pair(wa, wc, obs, M, ret, V, act, lp, stats, m, mean, std, ga, sums_a, gc, sums_c, st):
    ev = _ev_begin()
    _lib.check(_lib.lib().mhppo_mlp_train_pair(wa, wc, obs, M, ret, V, act, lp, stats, m, mean, std, ga, sums_a, gc,
                                               sums_c, st))
    _ev_end(ev, 3, 13, M)  # kind 3: a fused pair launch (two passes)


def k_mlp_train(kind, net, obs, ret, value=None, act=None, logp_old=None, stats=None, counts=None, m_global=1.0,
                exact=False, sums=None):
    """Fused forward/loss/backward of one head (mhppo_mlp_train), one validated call: the tests'
    and tools' entry (the update's drivers resolve a head's arguments once, _HeadPlan).
    kind 0 (critic): returns (grad, sums[3] = (sum (V-G)^2, sum A, sum A^2), V).
    kind 1 (continuous actor) / 2 (choice actor): returns (grad, sums[3] = (sum surrogate, 0, 0), None).
    grad is the packed torch-layout gradient (W1 b1 .. W4 b4), written into the net's flat
    .grad storage.  An empty `obs` (an empty data-parallel shard) gives a zero gradient.
    `sums`: optional zeroed float64 [3] the kernel accumulates into.
    exact: the f32-MFMA kernel instead of the split-precision one (any head with n_in <= 54;
    wider choice heads always run on f32 MFMA)."""
    _check_net(kind, net)
    dev = obs.device
    obs = _obs_rows(obs)
    M = obs.shape[0]
    ret = ret.float().contiguous()
    V = torch.empty(M, dtype=torch.float32, device=dev) if kind == KIND_CRITIC else value.detach().float().contiguous()
    act = None if act is None else act.float().contiguous()
    logp_old = None if logp_old is None else logp_old.float().contiguous()
    grad = net.grad_flat()
    if grad.numel() != n_params(net.n_in, net.n_out) or grad.device != dev:
        raise ValueError("gradient storage does not match the net / the batch's device")
    if sums is None:
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
    w = net.flat()
    with torch.cuda.device(dev):
        _launch_train(kind, TRAIN_EXACT_F32 if exact else 0, net.n_in, w.data_ptr(), obs.data_ptr(), M, ret.data_ptr(),
                      V.data_ptr(), _addr(act), _addr(logp_old), _addr(stats), _addr(counts), float(m_global),
                      float(net.mean), float(net.std), grad.data_ptr(), sums.data_ptr(),
                      torch.cuda.current_stream(dev).cuda_stream)
    return grad, sums, (V if kind == KIND_CRITIC else None)


def k_mlp_train_pair(actor, critic, obs, ret, value, act, logp_old, stats, m_global, sums_actor, sums_critic):
    """Actor pass of epoch e + critic pass of epoch e + 1 of one continuous head in one launch
    (mhppo_mlp_train_pair): `value` holds V_e (the critic pass e's outputs) and is overwritten
    with V_{e+1}; `stats` are the critic pass e's global advantage sums; the critic's weights
    must already carry its Adam step e.  Gradients go to both nets' flat .grad storage; the
    float64 sums accumulate into sums_actor / sums_critic (zeroed [3] each)."""
    _check_net(KIND_CONT, actor, pair=True)
    _check_net(KIND_CRITIC, critic, pair=True)
    dev = obs.device
    obs = _obs_rows(obs)
    M = obs.shape[0]
    ret, act, logp_old = ret.float().contiguous(), act.float().contiguous(), logp_old.float().contiguous()
    if value.dtype != torch.float32 or not value.is_contiguous() or value.numel() != M:
        raise ValueError("value must be the float32 [M] buffer of the previous critic pass (updated in place)")
    ga, gc = actor.grad_flat(), critic.grad_flat()
    wa, wc = actor.flat(), critic.flat()
    with torch.cuda.device(dev):
        _launch_pair(wa.data_ptr(), wc.data_ptr(), obs.data_ptr(), M, ret.data_ptr(), value.data_ptr(), act.data_ptr(),
                     logp_old.data_ptr(), _addr(stats), float(m_global), float(actor.mean), float(actor.std),
                     ga.data_ptr(), sums_actor.data_ptr(), gc.data_ptr(), sums_critic.data_ptr(),
                     torch.cuda.current_stream(dev).cuda_stream)
    return ga, gc, value


# ---------------------------------------------------------------- diagnostics
# mhppo_ppo_diag (include/mhppo.h MHPPO_DIAG_*): float64 sums over a head's batch
DIAG_DSUM, DIAG_K3, DIAG_CLIP, DIAG_RATIO, DIAG_ENT, DIAG_E, DIAG_E2, DIAG_G, DIAG_G2, DIAG_V = range(10)
DIAG_N = 10


def k_ppo_diag(head):
    """This rank's float64 [DIAG_N] diagnostic sums of one Head (mhppo_ppo_diag): the actor's and
    the critic's forward over head.obs with their current weights, against the batch's recorded
    act / logp / ret.  Forward only, one launch plus the fold, on the current stream; nothing is
    synchronised.  The scratch is allocated once per head (head._diag_work) and reused."""
    actor, critic = head.actor, head.critic
    want = 1 if head.kind == "c" else 2
    if actor.model_type != want or critic.model_type != 0:
        raise ValueError(f"a kind {head.kind!r} head has a model_type {want} actor and a model_type 0 critic")
    dev = head.obs.device
    obs = head.obs.float().contiguous()
    M = obs.shape[0]
    act = head.act.float().contiguous() if head.kind == "c" else head.act.to(torch.int32).contiguous()
    logp, ret = head.logp.float().contiguous(), head.ret.float().contiguous()
    L = _lib.lib()
    need = max(1, (int(L.mhppo_ppo_diag_work_bytes(M)) + 7) // 8)
    work = getattr(head, "_diag_work", None)
    if work is None or work.numel() < need or work.device != dev:
        work = head._diag_work = torch.empty(need, dtype=torch.float64, device=dev)
    sums = torch.empty(DIAG_N, dtype=torch.float64, device=dev)
    da, ka = actor.mlp_desc()
    dc, kc = critic.mlp_desc()
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(L.mhppo_ppo_diag(ctypes.byref(da), ctypes.byref(dc), p(obs), M, p(act), p(logp), p(ret), p(sums),
                                    p(work), _lib.stream_ptr()))
    return sums


def _kl_args(head):
    """(actor's mhppo_mlp, its backing tensor, obs, act, logp, M) of a Head as mhppo_ppo_kl reads them."""
    actor = head.actor
    want = 1 if head.kind == "c" else 2
    if actor.model_type != want:
        raise ValueError(f"a kind {head.kind!r} head has a model_type {want} actor")
    dev = head.obs.device
    if dev.type != "cuda":
        raise ValueError(f"the KL pass runs on the GPU only (there is no CPU path), not on {dev}")
    obs = head.obs.float().contiguous()
    act = head.act.float().contiguous() if head.kind == "c" else head.act.to(torch.int32).contiguous()
    da, keep = actor.mlp_desc()
    return da, keep, obs, act, head.logp.float().contiguous(), obs.shape[0]


def _kl_work(head, M, dev):
    need = max(1, (int(_lib.lib().mhppo_ppo_kl_work_bytes(M)) + 7) // 8)
    work = getattr(head, "_kl_work", None)
    if work is None or work.numel() < need or work.device != dev:
        work = head._kl_work = torch.empty(need, dtype=torch.float64, device=dev)
    return work


def k_ppo_kl(head, out=None):
    """This rank's float64 [2] KL sums of one Head (mhppo_ppo_kl): (sum d, sum (expm1(d) - d)),
    d = logp_new - logp_old, from the actor's forward over head.obs with its current weights --
    bit for bit k_ppo_diag(head)[:2], with neither the critic nor `ret` read.  Forward only, one
    launch plus the fold, on the current stream; nothing is synchronised.  out: a contiguous
    float64 [2] device tensor to write (default: a new one).  The scratch is allocated once per head
    (head._kl_work) and reused.  Not a train pass: it does not enter TRAIN_EVENTS."""
    da, keep, obs, act, logp, M = _kl_args(head)
    dev = obs.device
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=dev)
    elif out.dtype != torch.float64 or out.numel() != 2 or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous float64 [2] tensor on the head's device")
    work = _kl_work(head, M, dev)
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.ppo_kl(da, p(obs), M, p(act), p(logp), p(out), p(work), _lib.stream_ptr())
    return out


# The KL early stop's rule (Algo_PPO(target_kl=tau), train_epochs), as the gated Adam launch applies
# it on the device (include/mhppo.h mhppo_adam_clip_gated): its executable specification.
def kl_limit(target_kl, m):
    """The gate's bound on a head's GLOBAL K3 sum: 1.5 * target_kl * m (float64; m the global row
    count).  In sum units, so the kernel never divides: mean KL <= 1.5 tau  <=>  sum <= limit."""
    return 1.5 * float(target_kl) * float(m)


def kl_gate(kl_sum, limit, stop, epoch):
    """One gated net at one step: (open, stop').  open iff the net has not stopped (stop == 0) and
    kl_sum <= limit (a NaN fails the comparison and closes); the call that first closes the net
    records its epoch, and a stop is sticky.  A pure function."""
    is_open = stop == 0 and kl_sum <= limit
    return is_open, (stop if (is_open or stop != 0) else int(epoch))


def diag_stats(sums, m, entropy=True):
    """The per-iteration diagnostics of one head from its GLOBAL sums (a sequence of DIAG_N floats:
    all ranks' k_ppo_diag sums added) and global row count m.  A pure function.
    approx_kl: mean of expm1(d) - d, d = logp_new - logp_old (>= 0; the low-variance estimate of
    KL(old || new)); kl_k1 = -mean d; clip_frac: the rows whose ratio left [0.8, 1.2]; ratio_mean;
    entropy (choice head only: entropy=True); value_mse = mean (G - V)^2; explained_var =
    1 - Var(G - V) / Var(G), NaN when the returns have no variance."""
    s = [float(x) for x in sums]
    m = float(m)
    out = {"approx_kl": s[DIAG_K3] / m, "kl_k1": -s[DIAG_DSUM] / m, "clip_frac": s[DIAG_CLIP] / m,
           "ratio_mean": s[DIAG_RATIO] / m}
    if entropy:
        out["entropy"] = s[DIAG_ENT] / m
    out["value_mse"] = s[DIAG_E2] / m
    var_e = s[DIAG_E2] / m - (s[DIAG_E] / m) ** 2
    var_g = s[DIAG_G2] / m - (s[DIAG_G] / m) ** 2
    out["explained_var"] = 1.0 - var_e / var_g if var_g > 0.0 else math.nan
    return out


# ------------------------------------------------------------- DP orchestration

class Head:
    """One actor/critic pair, its Adam optimisers and this rank's shard of its batch.
    kind "c": continuous head (train_model_c, :778-815); "d": choice head (train_model_d,
    :818-851) with the GLOBAL action counts (n0, n1) of the M x M broadcast, or the
    opt-in per-row loss.  m = the global row count.  exact: the head's passes on
    the exact f32-MFMA kernel (Algo_PPO(exact_f32=True))."""

    def __init__(self, kind, actor, critic, opt_actor, opt_critic, obs, act, logp, ret, m, counts=None,
                 per_row=False, exact=False):
        self.kind, self.actor, self.critic = kind, actor, critic
        self.opt_actor, self.opt_critic = opt_actor, opt_critic
        self.obs, self.act, self.logp, self.ret, self.m = obs, act, logp, ret, float(m)
        self.counts = None if counts is None else counts.double().contiguous()
        self.per_row = per_row
        self.exact = bool(exact)


# Fuse each continuous head's actor pass e with its critic pass e + 1 (train_epochs) when the head
# has at most PAIR_MAX_ROWS rows (global).  The fused launch shares one input load and saves a
# launch, a weight-staging prologue and a reduction pair per epoch, but with two nets in one wave
# neither can hold its weight fragments in registers: per tile it is 3.6 % slower than the two
# passes (profiles/r04_pair/).  Measured end to end: config 2 (328 k rows per head) 7.92 -> 7.53
# ms per iteration, config 3 (10.5 M rows) 81.9 -> 85.9 ms.  MHPPO_PIPELINE_PAIRS=0 / =1 forces
# it off / on (A/B).
PIPELINE_PAIRS = {"0": False, "1": True}.get(os.environ.get("MHPPO_PIPELINE_PAIRS", ""), None)
PAIR_MAX_ROWS = 2_000_000


def _use_pair(h):
    if h.kind != "c" or h.exact:
        return False
    return PIPELINE_PAIRS if PIPELINE_PAIRS is not None else h.m <= PAIR_MAX_ROWS


class _HeadPlan:
    """One head's launch arguments for a whole train_epoch / train_epochs call, resolved once: the
    nets checked, the batch as contiguous float32 (16-byte aligned rows), the nets' flat weight /
    gradient pointers (fixed while the epochs run: the fused Adam updates them in place) and one V
    buffer.  Per pass only the stats / sums pointers change — the Python cost of a pass is one
    ctypes call (a per-call validation as in k_mlp_train, ~60 us of host time, left the GPU idle
    on small batches).  A head with no local rows (an empty data-parallel shard) has a plan too:
    with M == 0 the entry points zero the gradient and touch nothing else (include/mhppo.h)."""

    def __init__(self, h):
        cont = h.kind == "c"
        self.akind = KIND_CONT if cont else KIND_CHOICE
        _check_net(KIND_CRITIC, h.critic)
        _check_net(self.akind, h.actor)
        self.obs, self.ret = _obs_rows(h.obs), h.ret.float().contiguous()
        self.M = self.obs.shape[0]
        self.lp = h.logp.float().contiguous()
        # a choice head passes its global counts, or with the per-row loss its actions: never both
        self.act = h.act.float().contiguous() if (cont or h.per_row) else None
        self.counts = None if (cont or h.per_row) else h.counts
        self.V = torch.empty(self.M, dtype=torch.float32, device=self.obs.device)
        self.n_in = h.actor.n_in
        self.keep = (h.actor.flat(), h.critic.flat())  # the storages the pointers below point into
        self.wa, self.wc = self.keep[0].data_ptr(), self.keep[1].data_ptr()
        self.ga, self.gc = h.actor.grad_flat().data_ptr(), h.critic.grad_flat().data_ptr()
        self.mean, self.std = float(h.actor.mean), float(h.actor.std)
        self.flags = TRAIN_EXACT_F32 if h.exact else 0
        # an empty shard's actor and critic passes stay two launches (the launch record's rows)
        self.pair = _use_pair(h) and self.M > 0
        self.x, self.r, self.v, self.l = (t.data_ptr() for t in (self.obs, self.ret, self.V, self.lp))
        self.a, self.cn = _addr(self.act), _addr(self.counts)


# The three pass helpers of train_epoch / train_epochs, the only way the drivers reach the kernels
# (module-level names looked up at call time, so CPU test doubles can stand in for them:
# tests/test_dp_gloo.py).  sums / stats are float64 views: [3] rows of the step's sums, [2] stats;
# st is the hipStream_t handle of the current stream.
def _critic_pass(p, h, sums, st):
    _launch_train(KIND_CRITIC, p.flags, p.n_in, p.wc, p.x, p.M, p.r, p.v, None, None, None, None, h.m, 0.0, 1.0, p.gc,
                  sums.data_ptr(), st)


def _actor_pass(p, h, stats, sums, st):
    _launch_train(p.akind, p.flags, p.n_in, p.wa, p.x, p.M, p.r, p.v, p.a, p.l, stats.data_ptr(), p.cn, h.m, p.mean,
                  p.std, p.ga, sums.data_ptr(), st)


def _pair_pass(p, h, stats, sums_a, sums_c, st):
    _launch_pair(p.wa, p.wc, p.x, p.M, p.r, p.v, p.a, p.l, stats.data_ptr(), h.m, p.mean, p.std, p.ga,
                 sums_a.data_ptr(), p.gc, sums_c.data_ptr(), st)


def _on_device(dev):
    return torch.cuda.device(dev) if dev.type == "cuda" else contextlib.nullcontext()


def _reduce_and_step(nets, opts, bucket, max_grad_norm, norms_out, gates=None):
    """A step's epilogue: the gradient all-reduce of `nets` (in the bucket, or packed), then one
    adam_steps call over `opts`, their optimisers in the driver's order, clipped when max_grad_norm
    is set (norms_out: float64, contiguous, one element per optimiser, or None; gates: the KL early
    stop's gate table of the step, adam.gate_table)."""
    if bucket is not None:
        bucket.allreduce(nets)
    else:
        _allreduce_net_grads(*nets)
    if max_grad_norm is None:
        adam_steps(opts)
    elif opts and gates is None:
        adam_steps(opts, max_grad_norm, norms_out)
    elif opts:
        adam_steps(opts, max_grad_norm, norms_out, gates)


def train_epoch(heads, bucket=None, max_grad_norm=None, norms_out=None):
    """One full-batch epoch of every head: critic passes -> ONE all-reduce of all heads'
    advantage sums -> actor passes -> ONE gradient all-reduce -> Adam.  Returns this rank's
    (actor, critic) loss sums per head (float64 [1] tensors).  The sequential schedule
    train_epochs' pipeline is compared with, on the same plans and pass helpers.
    max_grad_norm (opt-in, adam_clip_steps): every net's gradient is clipped to that norm before
    its step.  The clip runs after the gradient all-reduce: the reduced gradient is replicated, so
    every rank measures the same norm and no further collective is needed.  norms_out: float64
    [2 H], receives the norms before clipping in the order (head 0's actor, head 0's critic, ...)."""
    H = len(heads)
    dev = heads[0].obs.device
    with _on_device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
        sums = torch.zeros(2 * H, 3, dtype=torch.float64, device=dev)  # critic rows, actor rows
        plans = [_HeadPlan(h) for h in heads]
        for i, (p, h) in enumerate(zip(plans, heads)):
            _critic_pass(p, h, sums[i], st)
        stats = sums[:H, 1:3].reshape(-1).contiguous()
        _allreduce_(stats)
        for i, (p, h) in enumerate(zip(plans, heads)):
            _actor_pass(p, h, stats[2 * i:2 * i + 2], sums[H + i], st)
        _reduce_and_step([n for h in heads for n in (h.actor, h.critic)],
                         [o for h in heads for o in (h.opt_actor, h.opt_critic)], bucket, max_grad_norm, norms_out)
    return [(sums[H + i, 0:1], sums[i, 0:1]) for i in range(H)]


# Heads' passes on alternating streams within an epoch step (train_epochs): head i's passes on
# stream i % TRAIN_STREAMS (a head's actor and critic passes stay in order on one stream: the critic
# pass e + 1 overwrites the V_e the actor pass e reads).  The heads are independent within a step, so
# one head's launch and weight staging overlap the other's tail, partial fold and reduction
# (mhppo_mlp_train keeps a workspace per stream).  Measured -0.7 % per iteration with two streams
# (profiles/r04_streams/), but then each kernel's execution span (rocprofv3) includes the time its
# blocks wait behind the other stream's kernel, so the per-kernel profile no longer matches the
# kernel's own duration: the default stays one stream; MHPPO_TRAIN_STREAMS=2 opts in.
TRAIN_STREAMS = max(1, int(os.environ.get("MHPPO_TRAIN_STREAMS", "1")))
_SIDE_STREAMS = {}


def _side_streams(dev, n):
    if dev.type != "cuda" or n <= 0:
        return []
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), n)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = [torch.cuda.Stream(device=dev) for _ in range(n)]
    return _SIDE_STREAMS[key]


class _KLPlan:
    """One head's mhppo_ppo_kl arguments for a whole gated train_epochs call, resolved once (the
    actor's descriptor points at its live flat weights, which Adam updates in place)."""

    def __init__(self, h):
        self.desc, *self.keep, self.M = _kl_args(h)
        obs, act, lp = self.keep[1:]
        self.keep.append(_kl_work(h, self.M, obs.device))
        self.x, self.a, self.l, self.w = (_lib.ptr(t) for t in (obs, act, lp, self.keep[-1]))

    def launch(self, out, st):
        _lib.ppo_kl(self.desc, self.x, self.M, self.a, self.l, out.data_ptr(), self.w, st)


def train_epochs(heads, n_epochs, bucket=None, max_grad_norm=None, target_kl=None):
    """n_epochs full-batch epochs of every head, run as a pipeline of n_epochs + 1 steps: step k
    runs the actor passes of epoch k - 1 and the critic passes of epoch k (a continuous head on the
    split-precision kernel: ONE fused launch, mhppo_mlp_train_pair), then one gradient all-reduce
    of the nets trained in the step, one all-reduce of the new critic passes' advantage sums and
    the Adam steps.  The same arithmetic as n_epochs calls of train_epoch: the actor of epoch e
    uses V_e and the advantage sums of the critic pass e (critic weights of epoch e), the critic
    of epoch e + 1 the critic's weights after its Adam step e; each optimiser steps n_epochs
    times.  Returns this rank's (actor, critic) loss sums of the last epoch per head.
    The launches go straight through the C-ABI with each head's arguments resolved once
    (_HeadPlan); an empty head (M == 0) runs the same passes, never paired: each zeroes a gradient.
    The float64 sums of all steps are one tensor [n_epochs + 1, 2 H, 3] (one fill, not one per
    step), and without data parallelism a head's advantage sums are read where its critic pass
    left them (all_sums[k - 1, i, 1:3], two contiguous doubles: no copy).
    max_grad_norm (opt-in, adam_clip_steps): every step's gradients are clipped to that norm per
    net, after the gradient all-reduce (the reduced gradient is replicated: every rank measures the
    same norm, no collective), and the call returns (losses, norms): norms float64 [n_epochs, 2 H]
    on the device, norms[e, j] the norm before clipping of head j's critic at its epoch e,
    norms[e, H + j] of head j's actor; NaN where a net was not stepped.  The launches fill it in
    place, without a host read: step k's nets are (actors of epoch k - 1, critics of epoch k),
    which in this layout are 2 H consecutive doubles starting at row k - 1, column H.
    target_kl (opt-in, the KL early stop; None: not a line of the above changes): a float tau > 0
    (inf measures and never stops).  Spinning Up's rule: the policy stops, the value function does
    not.  With theta_e the actor after e Adam steps and KL_e = (1 / m) sum (expm1(d) - d) over the
    head's whole batch under theta_e, the actor's step e (e = 1 .. n_epochs - 1; step 0 is never
    gated) is taken iff the head has not stopped and KL_e <= 1.5 tau (kl_gate; NaN stops); a stop
    is sticky for the rest of the call; the critics take all their steps.  So a head that stops
    at e has the actor of an e-epoch update and the critic of the full one.  Schedule: pipeline
    step k >= 2 first launches mhppo_ppo_kl per head (on the head's stream, after step k - 1's
    Adam) into kl[k - 2]; under data parallelism kl[k - 2] rides in the step's advantage-sum
    all-reduce (still two collectives per step; the last step, which has no critic pass, reduces it
    alone), so every rank decides alike; the step's one Adam launch is mhppo_adam_clip_gated with the
    actors gated by (kl[k - 2, i], kl_limit(tau, m_i), stop[i], epoch k - 1) and the critics
    ungated, max_norm inf when max_grad_norm is None.  The gate is decided on the device: nothing is
    read back, there is no host synchronisation between the loop's first and last launch.  Every
    step then runs on the native launch, which differs from torch._fused_adam_ by the rounding of
    the two bias corrections (include/mhppo.h).  The train passes of a stopped actor still run and
    their gradient is discarded: skipping them needs a host decision or an exit in the train
    kernel.  Returns (losses, norms, kl, stop): norms as above, or None when max_grad_norm is
    None; kl float64 [n_epochs - 1, H, 2] on the device, the GLOBAL (sum d, sum (expm1(d) - d)) of
    theta_e in kl[e - 1, i] (after a head's stop its rows repeat: the actor no longer moves);
    stop int32 [H], the actor steps taken when head i stopped (1 .. n_epochs - 1), 0 if it never did.
    Step counts: the clip records of the actors' optimisers are built before the loop (one host
    read each where missing) and dropped after it (clip_forget): a closed gate takes no step, so
    the host-side count runs ahead of the state's `step` tensor, which stays the truth."""
    H = len(heads)
    dev = heads[0].obs.device
    gated = target_kl is not None
    if gated:
        tau = float(target_kl)
        if not tau > 0.0:  # (NaN fails the comparison)
            raise ValueError(f"target_kl must be None or a float > 0 (inf allowed), not {target_kl!r}")
        if any(h.obs.device.type != "cuda" for h in heads):
            raise ValueError("target_kl needs every head on a GPU: the KL pass and the gate have no CPU path")
    with _on_device(dev):
        norms = None
        if max_grad_norm is not None or gated:
            norms = torch.full((n_epochs, 2 * H), math.nan, dtype=torch.float64, device=dev)
        if gated:
            kl = torch.zeros(max(0, n_epochs - 1), H, 2, dtype=torch.float64, device=dev)
            stop = torch.zeros(H, dtype=torch.int32, device=dev)
            klp = [_KLPlan(h) for h in heads]
            limits = [kl_limit(tau, h.m) for h in heads]
            clip_prepare([h.opt_actor for h in heads])
        all_sums = torch.zeros(n_epochs + 1, 2 * H, 3, dtype=torch.float64, device=dev)
        dp = _dp()
        plans = [_HeadPlan(h) for h in heads]
        main = torch.cuda.current_stream(dev) if dev.type == "cuda" else None
        side = _side_streams(dev, min(TRAIN_STREAMS, H) - 1)
        streams = [main] + side
        handles = [None if s is None else s.cuda_stream for s in streams]
        same_stream = contextlib.nullcontext()
        stats = None        # all-reduced advantage sums of the previous step's critic passes [2H]
        out = [[None, None] for _ in range(H)]
        for k in range(n_epochs + 1):
            sums = all_sums[k]  # critic rows, actor rows
            crit = k < n_epochs
            trained = []
            if side:  # the side streams start after this step's inputs (Adam, sums, stats) on main
                fork = torch.cuda.Event()
                fork.record(main)
                for sd in side:
                    sd.wait_event(fork)
            for i, h in enumerate(heads):
                p = plans[i]
                sc, sa = sums[i], sums[H + i]
                j = i % len(streams)
                st = handles[j]
                # (one stream: main is the current stream already; the launch events record on it)
                with (torch.cuda.stream(streams[j]) if side else same_stream):
                    if gated and k >= 2:  # KL of the actor after its k - 1 steps, ahead of its pass
                        klp[i].launch(kl[k - 2, i], st)
                    stp = None
                    if k > 0:  # the previous step's critic pass sums (all-reduced under data parallelism)
                        stp = stats[2 * i:2 * i + 2] if dp else all_sums[k - 1, i, 1:3]
                    if k > 0 and crit and p.pair:
                        _pair_pass(p, h, stp, sa, sc, st)
                    else:
                        if k > 0:  # the actor pass of epoch k - 1
                            _actor_pass(p, h, stp, sa, st)
                        if crit:  # the critic pass of epoch k
                            _critic_pass(p, h, sc, st)
                if k > 0:
                    trained.append(h.actor)
                    out[i][0] = sums[H + i, 0:1]
                if crit:
                    trained.append(h.critic)
                    out[i][1] = sums[i, 0:1]
            for sd in side:  # join
                main.wait_stream(sd)
            klk = kl[k - 2] if gated and k >= 2 else None
            if crit and dp and klk is not None:  # the KL sums ride with the advantage sums: one collective
                buf = torch.cat([sums[:H, 1:3].reshape(-1), klk.reshape(-1)])
                _allreduce_(buf)
                stats = buf[:2 * H]
                klk.copy_(buf[2 * H:].view(H, 2))
            elif crit and dp:  # the all-reduce needs one span
                stats = sums[:H, 1:3].reshape(-1).contiguous()
                _allreduce_(stats)
            elif dp and klk is not None:  # the last step: no critic pass, the KL sums alone
                _allreduce_(klk)
            # all H actors (k > 0), then all H critics (k < n_epochs)
            opts = ([h.opt_actor for h in heads] if k > 0 else []) + ([h.opt_critic for h in heads] if crit else [])
            nout = None
            if norms is not None:
                off = (k - 1) * 2 * H + H if k > 0 else 0
                nout = norms.view(-1)[off:off + len(opts)]
            if not gated:
                _reduce_and_step(trained, opts, bucket, max_grad_norm, nout)
                continue
            # the actors of step k >= 2 are gated by the KL of their k - 1 steps; step 0 (k == 1) and the critics never
            ent = [None] * len(opts)
            if klk is not None:
                ent[:H] = [(klk[i].data_ptr(), limits[i], stop[i].data_ptr(), k - 1) for i in range(H)]
            _reduce_and_step(trained, opts, bucket, math.inf if max_grad_norm is None else max_grad_norm, nout,
                             gate_table(ent))
        if gated:
            clip_forget([h.opt_actor for h in heads])
    if gated:
        return [tuple(o) for o in out], (norms if max_grad_norm is not None else None), kl, stop
    if norms is not None:
        return [tuple(o) for o in out], norms
    return [tuple(o) for o in out]


# ------------------------------------------------------------- minibatches (opt-in)

class _SliceHead:
    """What the pass helpers read of a Head, for one slice: the nets and the slice's GLOBAL row count."""

    def __init__(self, h, m):
        self.actor, self.critic, self.kind, self.m = h.actor, h.critic, h.kind, float(m)


class _SlicePlan:
    """Rows [b0, b1) of a _HeadPlan on the shuffled buffers: the same nets, the tensors as views
    (what the CPU doubles read) and the integer addresses offset by b0 rows (what the launchers
    read); b0 is a multiple of 4 rows, so X stays 16-byte aligned.  counts: the slice's global
    (n0, n1), two doubles of the call's counts buffer, or None."""

    def __init__(self, p, b0, b1, counts):
        for k in ("akind", "n_in", "wa", "wc", "ga", "gc", "mean", "std", "flags", "keep"):
            setattr(self, k, getattr(p, k))
        self.pair = False
        self.M = b1 - b0
        self.obs, self.ret, self.V, self.lp = p.obs[b0:b1], p.ret[b0:b1], p.V[b0:b1], p.lp[b0:b1]
        self.act = None if p.act is None else p.act[b0:b1]
        self.counts = counts
        self.x, self.r, self.v, self.l = p.x + 4 * self.n_in * b0, p.r + 4 * b0, p.v + 4 * b0, p.l + 4 * b0
        self.a = None if p.a is None else p.a + 4 * b0
        self.cn = _addr(counts)


def train_minibatches(heads, n_epochs, K, key_fn, bucket=None, max_grad_norm=None, slice_m=None):
    """n_epochs epochs of K minibatch steps per head (opt-in, Algo_PPO(minibatches=K); the reference
    and train_epochs run full-batch epochs).  Per epoch every head's batch is shuffled once, from the
    ORIGINAL tensors into the call's one shuffled copy, under key_fn(epoch, i) (i: the head's
    position in `heads`; mhppo.shuffle: a stateless keyed permutation, mhppo_batch_shuffle on the
    GPU); the copy is cut into K slices (mhppo.shuffle.slice_bounds) and step j of the epoch is
    EXACTLY train_epoch on slice j of every head: critic passes -> one all-reduce of the advantage
    sums -> actor passes -> gradient all-reduce -> Adam (clipped with max_grad_norm).  So m_global
    of a pass is the slice's global row count, the advantage is normalised per minibatch with the
    critic as it stands at that step, and the choice head gets its slice's global (n0, n1) (from
    the shuffle's per-slice counts), or its actions with the per-row loss.  Each optimiser steps
    n_epochs * K times, less the steps at which its head's slice is globally empty (M < 4 K): such
    a head is left out of the step, as update() leaves out an empty head; a locally empty slice
    runs with M == 0 and joins every collective.
    The driver is sequential on purpose: train_epochs' fused pair launch needs the actor pass and
    the next critic pass on the same rows, which holds for no two consecutive minibatches.
    The kernels are reached through _critic_pass / _actor_pass alone, one launcher call per pass
    with integer addresses resolved once per call (_HeadPlan on the shuffled copy, _SlicePlan).
    Data parallel: every rank shuffles its own shard and slices it by its local row count, so
    slice j is the union of the ranks' local slices j: a different draw of minibatches than one
    process on all envs would make (each is a uniform-looking sample of its shard; the results are
    not comparable run to run across world sizes, as the full-batch update's are).  Collectives: one
    all-reduce of the [H, K] local slice sizes per call (none when the caller passes slice_m, the
    GLOBAL sizes: update() joins it with its counts all-reduce), one of the choice heads' counts
    per epoch, and train_epoch's two per step.
    Returns per head (actor loss sum, critic loss sum, m) of the last step it was trained in (this
    rank's sums, float64 [1] tensors; m that step's global row count; None for a head never
    trained); with max_grad_norm also norms, float64 [n_epochs * K, 2 H] on the device in
    train_epochs' column layout (column j head j's critic, H + j its actor), NaN where a net was
    not stepped."""
    from . import shuffle
    H, K = len(heads), int(K)
    if K < 1:
        raise ValueError(f"K must be >= 1, not {K}")
    dev = heads[0].obs.device
    with _on_device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream if dev.type == "cuda" else None
        dp = _dp()
        n_choice = sum(1 for h in heads if h.kind != "c" and not h.per_row)
        counts_all = torch.zeros(max(1, n_choice), K, 2, dtype=torch.float64, device=dev)
        srcs, dsts, cnts, plans = [], [], [], []
        for h in heads:
            fl = h.kind == "c" or h.per_row  # the actions as the train kernel reads them, or int32 for the counts
            act = h.act.float().contiguous() if fl else h.act.to(torch.int32).contiguous()
            src = (h.obs.float().contiguous(), act, h.logp.float().contiguous(), h.ret.float().contiguous())
            dst = tuple(torch.empty_like(t) for t in src)
            cnt = None if fl else counts_all[sum(1 for c in cnts if c is not None)]
            srcs.append(src), dsts.append(dst), cnts.append(cnt)
            plans.append(_HeadPlan(Head(h.kind, h.actor, h.critic, h.opt_actor, h.opt_critic, *dst, h.m, cnt,
                                        h.per_row, h.exact)))
        bounds = [shuffle.slice_bounds(p.M, K) for p in plans]
        if slice_m is None:
            slice_m = [[float(b[j + 1] - b[j]) for j in range(K)] for b in bounds]
            if dp:  # one all-reduce and one host read per call
                slice_m = _allreduce_(torch.tensor(slice_m, dtype=torch.float64, device=dev)).tolist()
        sp = [[_SlicePlan(p, b[j], b[j + 1], None if c is None else c[j]) for j in range(K)]
              for p, b, c in zip(plans, bounds, cnts)]
        sh = [[_SliceHead(h, slice_m[i][j]) for j in range(K)] for i, h in enumerate(heads)]
        norms = None
        if max_grad_norm is not None:
            norms = torch.full((n_epochs * K, 2 * H), math.nan, dtype=torch.float64, device=dev)
        all_sums = torch.zeros(n_epochs * K, 2 * H, 3, dtype=torch.float64, device=dev)  # critic rows, actor rows
        out = [None] * H
        for e in range(n_epochs):
            for i in range(H):
                shuffle.shuffle_batch(srcs[i], dsts[i], key_fn(e, i), K, cnts[i])
            if n_choice:
                _allreduce_(counts_all)
            for j in range(K):
                on = [i for i in range(H) if slice_m[i][j] > 0]
                if not on:
                    continue
                sums = all_sums[e * K + j]
                for i in on:
                    _critic_pass(sp[i][j], sh[i][j], sums[i], st)
                stats = None
                if dp:  # the all-reduce needs one span
                    stats = sums[:H, 1:3].reshape(-1).contiguous()
                    _allreduce_(stats)
                for i in on:
                    _actor_pass(sp[i][j], sh[i][j], stats[2 * i:2 * i + 2] if dp else sums[i, 1:3], sums[H + i], st)
                    out[i] = (sums[H + i, 0:1], sums[i, 0:1], slice_m[i][j])
                nout = tmp = None
                if norms is not None:
                    if len(on) == H:
                        nout = norms[e * K + j]
                    else:
                        nout = tmp = torch.empty(2 * len(on), dtype=torch.float64, device=dev)
                # train_epochs' order within a step: the critics, then the actors
                _reduce_and_step([n for i in on for n in (heads[i].actor, heads[i].critic)],
                                 [heads[i].opt_critic for i in on] + [heads[i].opt_actor for i in on], bucket,
                                 max_grad_norm, nout)
                if tmp is not None:
                    norms[e * K + j, [i for i in on] + [H + i for i in on]] = tmp
    if norms is not None:
        return out, norms
    return out


def train_model_c(actor, critic, opt_actor, opt_critic, obs, act, logp_old, ret, m_global, exact=False):
    """One full-batch epoch of Algo_PPO.train_model_c (:778-815) for one head.
    Returns this rank's (actor, critic) loss sums (float64 tensors)."""
    return train_epoch([Head("c", actor, critic, opt_actor, opt_critic, obs, act, logp_old, ret, m_global,
                             exact=exact)])[0]


def train_model_d(actor, critic, opt_actor, opt_critic, obs, act, logp_old, ret, m_global, counts, per_row=False,
                  exact=False):
    """One full-batch epoch of Algo_PPO.train_model_d (:818-851) for one head: O(M) form of
    the M x M Categorical surrogate with the global action counts (n0, n1); per_row=True is
    the opt-in bug fix.  Returns this rank's (actor, critic) loss sums."""
    h = Head("d", actor, critic, opt_actor, opt_critic, obs, act, logp_old, ret, m_global, counts, per_row,
             exact=exact)
    return train_epoch([h])[0]
