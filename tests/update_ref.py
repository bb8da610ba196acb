"""A plain-torch restatement of one PPO update pass of a head (Algo_PPO.train_model_c / _d,
Coop-MH-PPO-scalable.py:778-851), in float64 by default, on whatever device its inputs are on.
Test infrastructure: it shares no code and no constant with mhppo.ppo's kernels (no ppo_math.h
branch table, no O(M) derivation in the literal choice loss), so it can judge them.

  Net            Model_PPO's forward on given weights, widened to `dtype`
  critic_pass    V, sum (V-G)^2, sum A, sum A^2 (A = G - V), gradient of mean (V-G)^2
  advantage      (A - mean) / (std_unbiased + 1e-10) from a given V and given advantage sums
  cont_pass      -min(r A, clamp(r, .8, 1.2) A) with r = exp(MVN(mu, 0.5).log_prob(act) - logp_old)
  choice_pass    the choice head's surrogate: "literal" (the reference program's M x M Categorical
                 broadcast, written as it stands), "counts" (its O(M) count-weighted form) or
                 "per_row" (the usual per-row surrogate)
Gradients come from torch.autograd.grad as one tensor per parameter (W1, b1, .., W4, b4);
split_packed slices a kernel's packed gradient the same way.  Every loss is `sum / m` (or
`sum / m^2`) with m the GLOBAL row count the kernels take as m_global, so a shard (M != m) has
the gradient of its rows' part of the global mean.

The same functions run in float32 (Net(..., dtype=torch.float32)): torch's own float32 autograd
of the same loss is the yardstick the kernel tests measure the kernels' float32 error against.
"""
import math

import torch

EPS = 2.0 ** -23                      # torch.finfo(float32).eps: Categorical's clamp of the probabilities
LN_LO, LN_HI = math.log(0.8), math.log(1.2)
LITERAL_MAX_ROWS = 1024               # the M x M tensor is built up to here (8 MiB of float64 per operand)
PARAM_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4")


def param_shapes(n_in, n_out):
    return [(32, n_in), (32,), (64, 32), (64,), (32, 64), (32,), (n_out, 32), (n_out,)]


def split_packed(flat, n_in, n_out):
    """A packed W1 b1 .. W4 b4 vector (the kernels' gradient layout) as one tensor per parameter."""
    shapes = param_shapes(n_in, n_out)
    total = sum(math.prod(s) for s in shapes)
    if flat.numel() != total:
        raise ValueError(f"packed size {flat.numel()} != {total} of a {n_in} -> {n_out} net")
    out, off = [], 0
    for shp in shapes:
        n = math.prod(shp)
        out.append(flat[off:off + n].reshape(shp))
        off += n
    return out


class Net:
    """in -> 32 -> 64 -> 32 -> out with ReLU on the given eight tensors (W1, b1, .., W4, b4; torch
    Linear layouts), cast to `dtype`.  kind 0: linear [M]; 1: tanh * std + mean [M]; 2: softmax over
    the output pair [M, 2]."""

    def __init__(self, params, kind, mean=0.0, std=1.0, dtype=torch.float64):
        if len(params) != 8:
            raise ValueError("eight tensors: W1 b1 W2 b2 W3 b3 W4 b4")
        self.params = [p.detach().to(dtype).clone().requires_grad_(True) for p in params]
        self.kind, self.mean, self.std, self.dtype = kind, float(mean), float(std), dtype
        self.n_in, self.n_out = self.params[0].shape[1], self.params[6].shape[0]

    @classmethod
    def of(cls, model, dtype=torch.float64):
        """From a Model_PPO (layer1..layer4, model_type, mean, std)."""
        ps = [q for lay in (model.layer1, model.layer2, model.layer3, model.layer4) for q in (lay.weight, lay.bias)]
        return cls(ps, model.model_type, model.mean, model.std, dtype)

    def preacts(self, x):
        """[z1, z2, z3, y]: every layer's output before its ReLU (y: before tanh / softmax)."""
        h, out = x.to(self.dtype), []
        for i in range(4):
            z = h @ self.params[2 * i].t() + self.params[2 * i + 1]
            out.append(z)
            h = torch.relu(z)
        return out

    def __call__(self, x, with_y=False):
        y = self.preacts(x)[3]
        if self.kind == 1:
            out = torch.tanh(y[:, 0]) * self.std + self.mean
        elif self.kind == 2:
            out = torch.softmax(y, dim=-1)
        else:
            out = y[:, 0]
        return (out, y) if with_y else out

    def grads(self, loss, y):
        """(the loss's gradient per parameter, the sum over rows of |dL/dy| per output).  The second is
        what b4's gradient, the plain sum over rows of dL/dy, would be without cancellation."""
        gs = torch.autograd.grad(loss, self.params + [y])
        return [g.detach() for g in gs[:8]], gs[8].detach().abs().sum(dim=0)


def surrogate(r, A):
    return -torch.minimum(r * A, torch.clamp(r, 0.8, 1.2) * A)


def critic_pass(net, obs, ret, m):
    """dict: V [M], sse = sum (V-G)^2, sum_a, sum_a2 (A = G - V), grads of sse / m (dy_abs: the sum
    over rows of |dL/dy|), v_terms: the largest row's sum of the magnitudes of the terms of the output
    dot product, sum_k |W4_k h3_k| + |b4| (what V would be without cancellation)."""
    z = net.preacts(obs)
    y = z[3]
    V = y[:, 0]
    with torch.no_grad():
        v_terms = ((torch.relu(z[2]) * net.params[6].abs()).sum(dim=1) + net.params[7].abs()).max()
    G = ret.to(net.dtype)
    sse = ((V - G) ** 2).sum()
    A = (G - V).detach()
    grads, dy_abs = net.grads(sse / m, y)
    return dict(V=V.detach(), sse=sse.detach(), sum_a=A.sum(), sum_a2=(A * A).sum(), sum_abs_a=A.abs().sum(),
                grads=grads, dy_abs=dy_abs, v_terms=v_terms)


def adv_sums(ret, V):
    """(sum A, sum A^2) of A = G - V in float64: what a critic pass hands the actor pass."""
    A = ret.double() - V.double()
    return torch.stack([A.sum(), (A * A).sum()])


def advantage(ret, V, stats, m, dtype=torch.float64):
    """(A - mean) / (std + 1e-10), torch.std's unbiased estimate, from the V and the advantage sums the
    kernel is given (so a critic's float32 error stays out of an actor comparison)."""
    s0, s1 = float(stats[0]), float(stats[1])
    mean = s0 / m
    var = (s1 - s0 * mean) / (m - 1.0)
    std = math.sqrt(max(var, 0.0))
    if dtype == torch.float64:
        return ((ret.double() - V.double()) - mean) / (std + 1e-10)
    mean_t = torch.tensor(mean, dtype=dtype, device=ret.device)
    std_t = torch.tensor(std, dtype=dtype, device=ret.device)
    return ((ret.to(dtype) - V.to(dtype)) - mean_t) / (std_t + 1e-10)


def cont_logp(net, obs, act, with_y=False):
    """MultivariateNormal(mu, [[0.5]]).log_prob(act) for the one-dimensional action: the Normal of
    variance 0.5 (no factorisation to run on the device; test_update_ref_host.py pins the two equal)."""
    mu, y = net(obs, True)
    lp = torch.distributions.Normal(mu, math.sqrt(0.5)).log_prob(act.to(net.dtype))
    return (lp, y) if with_y else lp


def cont_pass(net, obs, act, logp_old, A, m):
    """dict: surr = sum of the per-row surrogate (surr_abs: of its magnitudes), grads of surr / m,
    d = logp - logp_old."""
    lp, y = cont_logp(net, obs, act, True)
    d = lp - logp_old.to(net.dtype)
    f = surrogate(torch.exp(d), A.to(net.dtype))
    s = f.sum()
    grads, dy_abs = net.grads(s / m, y)
    return dict(surr=s.detach(), surr_abs=f.detach().abs().sum(), grads=grads, dy_abs=dy_abs, d=d.detach())


def choice_logits(net, obs, with_y=False):
    """log clamp(pn, eps, 1 - eps), pn = p / (p0 + p1): Categorical(probs=p).logits, [M, 2]."""
    p, y = net(obs, True)
    pn = p / p.sum(-1, keepdim=True)
    logits = torch.log(torch.clamp(pn, EPS, 1.0 - EPS))
    return (logits, y) if with_y else logits


def choice_pass(net, obs, logp_old, A, m, mode, act=None, counts=None):
    """dict: surr = the summed surrogate as the kernels report it (the loss times m^2; surr_abs: the
    sum of its entries' magnitudes), grads of the loss (dy_abs: the sum over rows of |dL/dy|, [2]),
    d = logits - logp_old [M, 2].
    mode "literal": logp[i, j] = logits[j, a_i], r[i, j] = exp(logp[i, j] - logp_old[j]), the sum over
      all M x M entries of -min(r A_j, clamp(r) A_j), over m^2 (needs act, M <= LITERAL_MAX_ROWS);
    mode "counts": sum_j sum_k counts[k] f(r_jk, A_j) / m^2;
    mode "per_row": sum_j f(r_j a_j, A_j) / m (its summed surrogate is reported times m)."""
    logits, y = choice_logits(net, obs, True)
    lpo, A = logp_old.to(net.dtype), A.to(net.dtype)
    M = obs.shape[0]
    if mode == "literal":
        if M > LITERAL_MAX_ROWS:
            raise ValueError("the literal M x M form is for M <= LITERAL_MAX_ROWS")
        a = act.long()
        logp = logits[:, a].t()                 # [i, j] = logits[j, a_i]
        r = torch.exp(logp - lpo[None, :])
        f = surrogate(r, A[None, :].expand(M, M))
        s = f.sum()
        loss = s / (m * m)
    elif mode == "counts":
        r = torch.exp(logits - lpo[:, None])
        f = surrogate(r, A[:, None].expand(M, 2)) * counts.to(net.dtype)[None, :]
        s = f.sum()
        loss = s / (m * m)
    elif mode == "per_row":
        lp = logits.gather(1, act.long()[:, None])[:, 0]
        f = surrogate(torch.exp(lp - lpo), A) * m
        s = f.sum()
        loss = s / (m * m)
    else:
        raise ValueError(mode)
    grads, dy_abs = net.grads(loss, y)
    return dict(surr=s.detach(), surr_abs=f.detach().abs().sum(), grads=grads, dy_abs=dy_abs,
                d=(logits - lpo[:, None]).detach())


def action_counts(act):
    return torch.stack([(act == 0).sum(), (act == 1).sum()]).double()


# ---- which rows a batch may hold: decided on the float64 forward alone, before any kernel runs
def away_from_kinks(nets, obs, tol=1e-4):
    """Rows none of whose hidden pre-activations, in any of `nets`, lies within `tol` of 0.  A ReLU's
    derivative jumps there: a float32 forward (the kernels', torch's) may take the other side than the
    float64 one, and the row's whole contribution to the gradient then differs, which is no error
    of either.  tol = 1e-4 is ~100 float32 roundings of a pre-activation of order 1."""
    keep = torch.ones(obs.shape[0], dtype=torch.bool, device=obs.device)
    with torch.no_grad():
        for net in nets:
            for z in net.preacts(obs)[:3]:
                keep &= (z.abs() > tol).all(dim=1)
    return keep


def away_from_clip(d, tol=1e-4):
    """Rows whose log-ratio(s) d = logp - logp_old lie further than `tol` from ln 0.8 and ln 1.2 (the
    surrogate's gradient jumps there; float32 rounding of logp moves d by ~1e-7 |logp|)."""
    k = ((d - LN_LO).abs() > tol) & ((d - LN_HI).abs() > tol)
    return k if k.dim() == 1 else k.all(dim=1)
