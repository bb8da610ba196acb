"""The optimiser steps of the PPO update (mhppo.ppo's drivers call adam_steps once per step):
adam_steps, all nets' fused torch Adam steps in 1 + (distinct lr) launches from a cached plan, and,
opt-in, adam_clip_steps: gradient-norm clipping and the Adam step of all nets in one native launch
(mhppo_adam_clip), with adam_clip_torch as its executable specification and CPU path."""
import contextlib
import math

import torch

from . import _lib


def _no_step_hooks(o):
    """No optimizer step hooks (per instance or global): the fast path bypasses Optimizer.step."""
    from torch.optim import optimizer as _opt
    return not (getattr(o, "_optimizer_step_pre_hooks", None) or getattr(o, "_optimizer_step_post_hooks", None)
                or getattr(_opt, "_global_optimizer_pre_hooks", None)
                or getattr(_opt, "_global_optimizer_post_hooks", None))


def _fused_adam_ok(o):
    return (hasattr(torch, "_fused_adam_") and hasattr(torch, "_foreach_add_") and _no_step_hooks(o)
            and isinstance(o, torch.optim.Adam) and getattr(o, "grad_scale", None) is None
            and getattr(o, "found_inf", None) is None
            and all(g.get("fused") and not g.get("amsgrad") and not g.get("capturable") and not g.get("differentiable")
                    and not g.get("decoupled_weight_decay", False) and not isinstance(g["lr"], torch.Tensor)
                    for g in o.param_groups))


class _AdamPlan:
    """The grouped tensor lists of one adam_steps(opts) call, reused while every optimiser keeps
    the same state / param_groups objects, hyper-parameters and .grad tensors (an optimiser's
    load_state_dict replaces those objects; a rebound .grad is a different tensor)."""

    def __init__(self, opts, keys, groups, steps, grads):
        self.opts, self.keys, self.groups, self.steps = opts, keys, groups, steps
        # strong references, compared by identity: an id() of a state dict freed by a later
        # load_state_dict could be reused by a newer one and pass a stale plan
        self.refs = [(o.state, o.param_groups) for o in opts]
        self.grads = grads  # [(param, grad)]

    def valid(self, opts):
        if len(opts) != len(self.refs) or not all(o.state is st and o.param_groups is pg
                                                  for o, (st, pg) in zip(opts, self.refs)):
            return False
        if _group_keys(opts) != self.keys or not all(_no_step_hooks(o) for o in opts):
            return False
        return all(p.grad is g for p, g in self.grads)


def _group_keys(opts):
    return [(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["weight_decay"]), float(g["eps"]),
             bool(g["maximize"])) for o in opts for g in o.param_groups]


_ADAM_PLANS = {}


def adam_steps(opts, max_grad_norm=None, norms_out=None, gates=None):
    """One step of every optimiser in `opts`.  max_grad_norm set (opt-in): every net's gradient is
    clipped to that norm first and the step runs on the native clip-and-Adam launch
    (adam_clip_steps below; norms_out and gates as there); the rest of this text is the default, None.

    Bit-identical to calling o.step() on each.  For
    fused torch Adams (the GPU path) whose state exists, the steps of all six nets run as ONE
    step-count increment and one torch._fused_adam_ launch per distinct hyper-parameter set —
    the same per-tensor kernel arithmetic as each optimiser's own step (torch.optim.adam
    _fused_adam), in 1 + (distinct lr) launches instead of 2 per optimiser.  Anything else (CPU,
    the first step, which creates the state, non-default options, registered optimizer step
    hooks, a torch without the private torch._fused_adam_ op) takes o.step().  The fast path
    reads each group's lr at every call, so an LR scheduler's changes apply; it does not run
    Optimizer.step itself (no step hooks — hence the fallback above — and no scheduler
    step-order bookkeeping).  The grouped tensor lists are built once per optimiser set and
    reused (_AdamPlan: ~0.2 ms of host time per call otherwise).  Pinned by
    test_adam_steps_bit_identical_to_per_optimizer_steps."""
    if max_grad_norm is not None:
        return adam_clip_steps(opts, max_grad_norm, norms_out, gates)
    if gates is not None:
        raise ValueError("gates need the native launch: pass max_grad_norm (inf clips nothing)")
    key = tuple(id(o) for o in opts)
    plan = _ADAM_PLANS.get(key)
    if plan is not None and plan.opts == list(opts) and plan.valid(opts):
        _run_adam_plan(plan)
        return
    fast = all(_fused_adam_ok(o) for o in opts)
    groups, steps, grads = {}, [], []
    if fast:
        for o in opts:
            for g in o.param_groups:
                ps = [p for p in g["params"] if p.grad is not None]
                if any(len(o.state[p]) == 0 for p in ps):
                    fast = False
                    break
                if not ps:
                    continue
                hk = (ps[0].device, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]),
                      float(g["weight_decay"]), float(g["eps"]), bool(g["maximize"]))
                e = groups.setdefault(hk, ([], [], [], [], []))
                for p in ps:
                    st = o.state[p]
                    if p.dtype != torch.float32 or p.device != hk[0]:
                        fast = False
                    e[0].append(p)
                    e[1].append(p.grad)
                    e[2].append(st["exp_avg"])
                    e[3].append(st["exp_avg_sq"])
                    e[4].append(st["step"])
                    steps.append(st["step"])
                    grads.append((p, p.grad))
            if not fast:
                break
    if not fast:
        _ADAM_PLANS.pop(key, None)
        for o in opts:
            o.step()
        return
    plan = _AdamPlan(list(opts), _group_keys(opts), groups, steps, grads)
    if len(_ADAM_PLANS) > 64:
        _ADAM_PLANS.clear()
    _ADAM_PLANS[key] = plan
    _run_adam_plan(plan)


def _run_adam_plan(plan):
    torch._foreach_add_(plan.steps, 1)
    for (_, lr, b1, b2, wd, eps, maximize), (ps, gs, ms, vs, sts) in plan.groups.items():
        torch._fused_adam_(ps, gs, ms, vs, [], sts, amsgrad=False, lr=lr, beta1=b1, beta2=b2, weight_decay=wd,
                           eps=eps, maximize=maximize, grad_scale=None, found_inf=None)


# ------------------------------------------------- gradient-norm clipping + Adam (opt-in)
# mhppo_adam_clip (include/mhppo.h, csrc/adam_clip.hip): per net the gradient norm in the fixed
# fold order, the clip scale and the Adam step on the torch optimiser's own state, all nets of a
# pipeline step in one launch.  adam_clip_torch is the contract's executable specification (the
# tests compare the kernel with it bit for bit) and the CPU path.

def fold_1024_4(x):
    """The fold of a float64 vector in k_fold<1024, 4>'s order (csrc/block_prims.h): thread b's
    chain u adds elements b + 1024 u (+ 4096 k) from +0.0, (a0 + a1) + (a2 + a3), the halving tree."""
    x = x.reshape(-1)
    n = x.numel()
    rounds = max(1, -(-n // 4096))
    pad = x.new_zeros(rounds * 4096)  # an absent element adds +0.0 to a chain that is never -0.0
    pad[:n] = x
    pad = pad.view(rounds, 4, 1024)
    acc = x.new_zeros(4, 1024)
    for r in range(rounds):
        acc = acc + pad[r]
    v = (acc[0] + acc[1]) + (acc[2] + acc[3])
    s = 512
    while s:
        v = v[:s] + v[s:2 * s]
        s //= 2
    return v[0]


def adam_clip_sumsq(grads):
    """ss of the contract: the squares of the net's flat gradient (the tensors of `grads` in
    order), exact in float64, folded in k_fold<1024, 4>'s order.  A float64 scalar tensor."""
    g = torch.cat([x.detach().reshape(-1) for x in grads]).double()
    return fold_1024_4(g * g)


def _f32(x):
    return torch.tensor(float(x), dtype=torch.float64).to(torch.float32)


def adam_clip_torch(segs, t, lr, beta1, beta2, eps, max_norm, norm=None):
    """mhppo_adam_clip's arithmetic for one net, operation for operation (include/mhppo.h), in
    place on torch tensors: segs = [(param, grad, exp_avg, exp_avg_sq, step)] in flat order, t the
    step count after the increment.  Returns the float64 norm before clipping (a Python float).
    norm: use this value instead of sqrt(ss) (the tests feed the kernel's reported norm, so that a
    last-bit difference of the float64 square root cannot move the comparison of the step)."""
    if norm is None:
        norm = math.sqrt(float(adam_clip_sumsq([s[1] for s in segs])))
    coef = float(max_norm) / (norm + 1e-6)
    s = _f32(coef) if coef < 1.0 else _f32(1.0)
    a, q = _f32(lr / (1.0 - beta1 ** t)), _f32(math.sqrt(1.0 - beta2 ** t))
    c1, b2, c2, e = _f32(1.0 - beta1), _f32(beta2), _f32(1.0 - beta2), _f32(eps)
    with torch.no_grad():
        for p, g, m, v, step in segs:
            p, g = p.detach(), g.detach()
            dev = p.device
            gs = g * s.to(dev)
            m.add_((gs - m) * c1.to(dev))
            v.mul_(b2.to(dev)).add_((gs * gs) * c2.to(dev))
            # sqrtf, correctly rounded: through float64 (a float32 root is never near enough to a
            # rounding boundary for the second rounding to matter); torch's float32 CPU sqrt is a
            # vectorised approximation that misses the IEEE result in ~0.6 % of the elements
            den = (v.double().sqrt().float() / q.to(dev)) + e.to(dev)
            p.sub_((m / den) * a.to(dev))
            step.fill_(float(t))
    return norm


def _clip_group_ok(g):
    return (not g.get("amsgrad") and not g.get("maximize") and not g.get("capturable")
            and not g.get("differentiable") and not isinstance(g["lr"], torch.Tensor)
            and float(g["weight_decay"]) == 0.0)


class _ClipNet:
    """One torch.optim.Adam as one net of a mhppo_adam_clip call: its parameters in order as the
    segments, the state tensors' addresses and the host-side step count t.  t is read from the
    state ONCE, when the record is built, and incremented per step; the record is rebuilt (and t
    read again) when the optimiser's `state` or `param_groups` object, a state dict, a parameter's
    storage or a `.grad` tensor is replaced (load_state_dict, .to(), zero_grad(set_to_none=True))
    or a step hook appears.  What it cannot see is a step taken behind its back on the same state
    objects (o.step(), adam_steps without max_grad_norm): clip_forget(opts) drops the records then.
    ok is False for an optimiser the kernel does not serve (see adam_clip_steps)."""

    def __init__(self, o):
        self.opt, self.state, self.pg = o, o.state, o.param_groups
        self.ok = False
        if not (isinstance(o, torch.optim.Adam) and _no_step_hooks(o) and len(o.param_groups) == 1
                and getattr(o, "grad_scale", None) is None and getattr(o, "found_inf", None) is None
                and _clip_group_ok(o.param_groups[0])):
            return
        g = o.param_groups[0]
        ps = [p for p in g["params"] if p.grad is not None]
        if not ps or len(ps) > _lib.ADAM_MAX_SEGS:
            return
        dev = ps[0].device
        if dev.type not in ("cuda", "cpu") or (dev.type == "cuda" and not g.get("fused")):
            return  # a foreach / single-tensor GPU optimiser keeps `step` on the host
        for p in ps:
            if (p.dtype != torch.float32 or p.device != dev or not p.is_contiguous() or p.grad.dtype != torch.float32
                    or p.grad.device != dev or not p.grad.is_contiguous()):
                return
        fresh = [p for p in ps if len(o.state[p]) == 0]
        for p in fresh:  # the state torch's Adam._init_group would create at the first step
            st = o.state[p]
            st["step"] = (torch.zeros((), dtype=torch.float32, device=dev) if g.get("fused")
                          else torch.tensor(0.0, dtype=torch.float32))
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        sts = [o.state[p] for p in ps]
        for p, st in zip(ps, sts):
            m, v, step = st.get("exp_avg"), st.get("exp_avg_sq"), st.get("step")
            if not (torch.is_tensor(m) and torch.is_tensor(v) and torch.is_tensor(step)) or step.numel() != 1:
                return
            if step.dtype != torch.float32 or (dev.type == "cuda" and step.device != dev):
                return
            for x in (m, v):
                if x.dtype != torch.float32 or x.device != dev or not x.is_contiguous() or x.numel() != p.numel():
                    return
        if len(fresh) == len(ps):
            ts = {0}
        else:  # one host read per optimiser and record
            ts = {int(x) for x in torch.stack([st["step"].reshape(()).to(dev) for st in sts]).tolist()}
        if len(ts) != 1:
            return
        self.t = ts.pop()
        self.dev = dev
        self.params = [(p, p.grad, p.data_ptr(), st) for p, st in zip(ps, sts)]
        self.segs = [(p, p.grad, st["exp_avg"], st["exp_avg_sq"], st["step"]) for p, st in zip(ps, sts)]
        self.ok = True

    def valid(self):
        o = self.opt
        if o.state is not self.state or o.param_groups is not self.pg or not _no_step_hooks(o):
            return False
        if not self.ok:
            return False  # an unsupported optimiser is looked at again at every call
        get = self.state.get
        return _clip_group_ok(self.pg[0]) and all(p.grad is g and p.data_ptr() == ptr and get(p) is st
                                                  for p, g, ptr, st in self.params)

    def hyper(self):
        """(t, lr, beta1, beta2, eps) of the step about to run: read at every call."""
        g = self.pg[0]
        return self.t + 1, float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])


_CLIP_NETS = {}    # id(optimiser) -> _ClipNet
_CLIP_PLANS = {}   # ids of an optimiser set -> (records, ctypes table)


def clip_forget(opts=None):
    """Drop the clip path's records of `opts` (default: all), so the next clipped step reads the
    step counts from the optimisers' state again."""
    for k in ([id(o) for o in opts] if opts is not None else list(_CLIP_NETS)):
        _CLIP_NETS.pop(k, None)
    _CLIP_PLANS.clear()


def _clip_net(o):
    rec = _CLIP_NETS.get(id(o))
    if rec is None or rec.opt is not o or not rec.valid():
        if len(_CLIP_NETS) > 256:
            clip_forget()
        rec = _CLIP_NETS[id(o)] = _ClipNet(o)
    return rec


def clip_prepare(opts):
    """Build the clip path's records of `opts` now (one host read of the step count per optimiser
    whose record is missing or stale), so that the steps that follow find them and read nothing."""
    for o in opts:
        _clip_net(o)


def _clip_table(recs):
    nets = (_lib.AdamNet * len(recs))()
    for net, rec in zip(nets, recs):
        net.n_seg = len(rec.segs)
        for sg, (p, g, m, v, step) in zip(net.seg, rec.segs):
            sg.param, sg.grad, sg.exp_avg, sg.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            sg.step, sg.n = step.data_ptr(), p.numel()
    return nets


def _clip_launch(recs, nets, max_norm, norms, gates=None):
    """One mhppo_adam_clip call for `recs` (all on one GPU) on the current stream; with `gates` (a
    ctypes array of _lib.AdamGate, one per record) one mhppo_adam_clip_gated call instead."""
    hs = [rec.hyper() for rec in recs]
    for net, (t, lr, b1, b2, eps) in zip(nets, hs):
        net.t, net.alpha, net.bias2 = t, lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)
        net.beta1, net.beta2, net.eps = b1, b2, eps
    dev = recs[0].dev
    with (contextlib.nullcontext() if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)):
        st = torch.cuda.current_stream(dev).cuda_stream
        if gates is None:
            _lib.adam_clip(nets, len(recs), max_norm, norms.data_ptr(), st)
        else:
            _lib.adam_clip_gated(nets, len(recs), max_norm, norms.data_ptr(), gates, st)
    for rec in recs:
        rec.t += 1


def gate_table(entries):
    """The host array of mhppo_adam_gate for one gated call: per optimiser None (not gated) or
    (kl address, limit, stop address, epoch): kl the device address of the net's two float64 KL
    sums, stop of its int32 stop word (include/mhppo.h)."""
    tab = (_lib.AdamGate * max(1, len(entries)))()
    for g, e in zip(tab, entries):
        if e is not None:
            g.kl, g.limit, g.stop, g.epoch = e[0], float(e[1]), e[2], int(e[3])
    return tab


def adam_clip_steps(opts, max_grad_norm, norms_out=None, gates=None):
    """adam_steps with the knob set: per optimiser (= per net) clip the gradient to max_grad_norm
    (> 0; inf clips nothing and only measures), then one Adam step.  Returns the float64 norms
    before clipping, one per optimiser in order, in norms_out (float64, contiguous,
    len(opts) elements, on the nets' device) or a new tensor; nothing is read back to the host.

    GPU: ONE mhppo_adam_clip launch for all optimisers of the call (include/mhppo.h has the
    arithmetic), on the optimisers' own state tensors: state_dict() and the checkpoints stay the
    truth.  The first step is native too: where torch has not created the Adam state yet it is
    created here as Adam._init_group would (zero moments, a float32 device scalar `step`).  The
    segment table is built once per optimiser set and reused under _AdamPlan's rule (identity of
    state / param_groups / .grad, plus the parameters' addresses; _ClipNet says what rebuilds it
    and what the host-side step count cannot see); lr, betas and eps are read at every call, so a
    scheduler's changes apply.  CPU tensors (the test doubles) take adam_clip_torch, the same
    arithmetic: CPU and GPU runs of one seed agree bit for bit in the optimiser.
    Fallback: an optimiser the kernel does not serve (not torch.optim.Adam, weight_decay, amsgrad,
    maximize, capturable, differentiable, a tensor lr, several param groups, more than 8 parameter
    tensors, non-float32 or non-contiguous tensors, a GPU optimiser that is not fused=True (its
    `step` lives on the host), step hooks) takes torch.nn.utils.clip_grad_norm_ on its
    parameters, then o.step(); the others of the call still go native, one launch each.
    gates (opt-in, the KL early stop: gate_table's array, one entry per optimiser): the one launch
    is mhppo_adam_clip_gated, and a net whose gate is closed on the device takes no step (its norm
    is NaN, its state keeps its bits).  The host-side step count of its record is then one ahead
    of the state's `step`: the caller drops the records (clip_forget) before that optimiser's next
    step.  Gates are served by the all-native launch alone: a CPU or unsupported optimiser raises."""
    max_norm = float(max_grad_norm)
    if not max_norm > 0.0:
        raise ValueError(f"max_grad_norm must be > 0 (inf allowed), not {max_grad_norm!r}")
    opts = list(opts)
    if not opts:
        return norms_out
    key = tuple(id(o) for o in opts)
    plan = _CLIP_PLANS.get(key)
    if plan is not None and all(_CLIP_NETS.get(k) is rec and rec.valid() for k, rec in zip(key, plan[0])):
        recs, nets = plan
    else:
        recs, nets = [_clip_net(o) for o in opts], None
        _CLIP_PLANS.pop(key, None)
    dev = recs[0].dev if recs[0].ok else next((p.device for p in opts[0].param_groups[0]["params"]), None)
    if norms_out is None:
        norms_out = torch.empty(len(opts), dtype=torch.float64, device=dev)
    elif norms_out.dtype != torch.float64 or not norms_out.is_contiguous() or norms_out.numel() != len(opts):
        raise ValueError("norms_out must be a contiguous float64 tensor with one element per optimiser")
    if all(r.ok and r.dev.type == "cuda" and r.dev == dev for r in recs) and norms_out.device == dev:
        if nets is None:
            nets = _clip_table(recs)
            if len(_CLIP_PLANS) > 64:
                _CLIP_PLANS.clear()
            _CLIP_PLANS[key] = (recs, nets)
        _clip_launch(recs, nets, max_norm, norms_out, gates)
        return norms_out
    if gates is not None:
        raise ValueError("a gated step needs fused torch.optim.Adam optimisers on one GPU (the gate is decided "
                         "on the device: there is no CPU path)")
    for k, (o, rec) in enumerate(zip(opts, recs)):
        if rec.ok and rec.dev.type == "cuda":
            one = norms_out[k:k + 1] if norms_out.device == rec.dev else torch.empty(1, dtype=torch.float64,
                                                                                     device=rec.dev)
            _clip_launch([rec], _clip_table([rec]), max_norm, one)
            if one.device != norms_out.device:
                norms_out[k:k + 1].copy_(one)
        elif rec.ok:
            t, lr, b1, b2, eps = rec.hyper()
            norms_out[k] = adam_clip_torch(rec.segs, t, lr, b1, b2, eps, max_norm)
            rec.t += 1
        else:
            ps = [p for g in o.param_groups for p in g["params"] if p.grad is not None]
            norms_out[k] = torch.nn.utils.clip_grad_norm_(ps, max_norm).detach().double()
            o.step()
    return norms_out
