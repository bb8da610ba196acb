"""The PPO heads' per-row arithmetic of csrc/ppo_heads.h, compiled for the host (tools/hostfwd.cpp
hf_*: the LibmUpdate flavour with the host's libm), on the CPU (no GPU):

  cat_normalise, cat_clamp     bit for bit against torch's Categorical(probs=...) normalisation and
                               clamp_probs (the logf after the clamp is the libm's: not pinned here);
  adv_moments, adv_normalised  bit for bit against torch.mean / torch.std (unbiased) of the float64
                               advantages rounded once, and against the float32 expression of
                               update_ref.advantage;
  cont_logp_x                  bit for bit against mvn_logp (the rounded exact difference of two floats
                               is their float32 difference);
  the loss rows                choice_term + cat_grad_p + softmax_jacobian, and cont_logp_x +
                               surr_and_grad(_fd) + cont_dmu + the tanh backward, chained as the train
                               kernels chain them (hf_choice_row, hf_cont_row), against float64 torch
                               autograd of update_ref's row losses (surrogate, cont_pass, choice_pass:
                               global counts and per row), from the head's last-layer output y on.

Bound of the loss rows, the scheme of test_update_matrix_gpu.py: err <= K * e32 + floor over the
rows' dL/dy, with err the max-abs error against float64, e32 that of torch's own float32 autograd of
the same rows and floor = 4 float32 ulps (4 * 2^-23) of max |dL/dy|.  K is twice the worst err / e32
measured on the CPU (4 096 rows drawn per case, seeds 0, 1, 2):
    cont, float64 ratio (the exact-f32 kernel's form)           0.92  0.30  3.20
    cont, float32 ratio + float64 clip decision (split kernel)   0.92  0.30  3.82    worst 3.82, K = 7.7
    choice, global counts                                        0.75  0.81  0.77
    choice, per row                                              0.92  0.91  0.88    worst 0.92, K = 1.9
(The max over a few thousand rows of one float32 rounding each: torch's e32 stayed at 0.2 to 1 times
the floor in every case, so the floor carries as much of the bound as K * e32 does; err was 1.6e-9 to
5.7e-9 for the continuous rows, 1.0e-10 to 4.1e-10 for the choice rows.)
Rows come from update_ref.away_from_clip (a row within 1e-4 of a clip bound may take the other
branch in float32, torch's as much as this code's); at least 90 % of the drawn rows must survive.
The clamp bounds pn = eps and pn = 1 - eps have a case of their own: torch.clamp passes the gradient
on the closed interval and gives exactly 0 outside, and so must choice_term's mask."""
import numpy as np
import pytest
import torch
from torch.distributions import Categorical
from torch.distributions.utils import clamp_probs

import infer_common as ic
import update_ref as ur

EPS32 = np.float32(2.0 ** -23)
HI32 = np.float32(1.0) - EPS32
FLOOR = 4 * 2.0 ** -23
K_CONT, K_CHOICE = 7.7, 1.9
M_ROWS = 4096


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f32(x):
    return np.float32(x)


# ------------------------------------------------------------ Categorical: normalise and clamp
def test_cat_normalise_and_clamp_bits():
    hf = ic.hostfwd()
    rng = np.random.default_rng(5)
    q = rng.random(4000, dtype=np.float32)
    pairs = [np.stack([q, f32(1.0) - q], 1),                               # softmax outputs
             rng.random((2000, 2), dtype=np.float32) * f32(7.0),            # unnormalised
             np.stack([f32(10.0) ** rng.uniform(-12, 0, 2000).astype(np.float32), np.ones(2000, np.float32)], 1)]
    below, above = np.nextafter(EPS32, f32(0)), np.nextafter(EPS32, f32(1))
    hi_in, hi_out = np.nextafter(HI32, f32(0)), np.nextafter(HI32, f32(2))   # hi_out = 1
    edge = [(0, 1), (1, 0), (EPS32, HI32), (HI32, EPS32), (below, 1), (above, 1), (1, below), (below, hi_out),
            (above, hi_in), (EPS32, 1), (2, 6), (1e-30, 3), (0.25, 0.25), (3e-8, 0.5), (1e-7, 1e-7), (5, 5e-7),
            (below, HI32), (EPS32 * 2, 2)]
    pairs.append(np.array(edge, np.float32))
    p = np.concatenate(pairs)
    t = torch.from_numpy(p)
    ref_n = Categorical(probs=t, validate_args=False).probs
    assert ref_n.dtype == torch.float32
    pn, sp = hf.cat_normalise(p)
    assert np.array_equal(bits32(pn), bits32(ref_n.numpy()))
    assert np.array_equal(bits32(sp), bits32((t[:, 0] + t[:, 1]).numpy()))
    # the clamp on the normalised pairs and on the bounds' neighbours themselves
    vals = np.concatenate([pn.ravel(), np.array([0, 1, EPS32, HI32, below, above, hi_in, hi_out], np.float32)])
    ref_c = clamp_probs(torch.from_numpy(vals)).numpy()
    got = hf.cat_clamp(vals)
    assert np.array_equal(bits32(got), bits32(ref_c))
    assert (vals < EPS32).sum() > 10 and (vals > HI32).sum() > 10  # both sides of the clamp are exercised
    assert got.min() == EPS32 and got.max() == HI32


# ------------------------------------------------------------ the advantage's normalisation
@pytest.mark.parametrize("loc,scale", [(0.3, 1.0), (-2.0, 1e-3), (5e-5, 1e-6), (40.0, 7.0)])
def test_adv_moments_and_normalised_bits(loc, scale):
    hf = ic.hostfwd()
    rng = np.random.default_rng(17)
    m = 5000
    ret = (loc + scale * rng.standard_normal(m)).astype(np.float32)
    V = (0.1 * scale * rng.standard_normal(m)).astype(np.float32)
    a = ret - V                                   # float32, as the kernels form it
    a64 = torch.from_numpy(a).double()
    stats = torch.stack([a64.sum(), (a64 * a64).sum()])
    meanf, stdf = hf.adv_moments(stats.numpy(), float(m))
    assert bits32(meanf) == bits32(a64.mean().float().numpy())
    assert bits32(stdf) == bits32(a64.std(unbiased=True).float().numpy())
    got = hf.adv_normalised(a, meanf, stdf)
    ref = ur.advantage(torch.from_numpy(ret), torch.from_numpy(V), stats, float(m), dtype=torch.float32)
    assert ref.dtype == torch.float32
    assert np.array_equal(bits32(got), bits32(ref.numpy()))
    # the float32 expression written out: (A - mean) / (std + 1e-10), every operation in float32
    ref2 = (a - meanf) / (stdf + np.float32(1e-10))
    assert ref2.dtype == np.float32 and np.array_equal(bits32(got), bits32(ref2))


def test_adv_moments_degenerate_variance_is_clamped():
    hf = ic.hostfwd()
    meanf, stdf = hf.adv_moments(np.array([3.0, 3.0 - 1e-12]), 3.0)  # sum A^2 < (sum A)^2 / m by rounding
    assert meanf == np.float32(1.0) and stdf == np.float32(0.0)


# ------------------------------------------------------------ the two forms of the MVN log-prob
def test_cont_logp_x_equals_mvn_logp_bits():
    hf = ic.hostfwd()
    rng = np.random.default_rng(23)
    n = 20000
    mu = (3.0 * rng.standard_normal(n) - 1.0).astype(np.float32)
    act = (mu + np.sqrt(0.5) * rng.standard_normal(n)).astype(np.float32)
    # exponents far apart (the exact difference needs more than 53 bits), close values, signed zeros,
    # subnormals
    big = (rng.standard_normal(2000) * 10.0 ** rng.uniform(-38, 18, 2000)).astype(np.float32)
    small = (rng.standard_normal(2000) * 10.0 ** rng.uniform(-45, 3, 2000)).astype(np.float32)
    tiny = np.float32(1e-45)
    e_a = np.array([0.0, -0.0, 0.0, 1.0, 1.0, tiny, -tiny, 3e-39, 1.5, 16777216.0, 1e18, -1e18, 1.0], np.float32)
    e_m = np.array([0.0, 0.0, -0.0, np.nextafter(f32(1), f32(2)), 1.0, -tiny, tiny, 1e-39, tiny, 0.5, 1.0, 1e-30,
                    2.0 ** -25], np.float32)
    a = np.concatenate([act, big, small, mu[:2000], e_a])
    b = np.concatenate([mu, small, big, np.nextafter(mu[:2000], np.float32(np.inf)), e_m])
    lp, x = hf.cont_logp_x(a, b)
    assert np.isfinite(lp).all()
    assert np.array_equal(bits32(lp), bits32(hf.mvn_logp(a, b)))
    assert np.array_equal(bits32(x), bits32((a - b) * np.float32(float.fromhex("0x1.6a09e6p+0"))))


# ------------------------------------------------------------ loss rows against float64 autograd
class YHead(ur.Net):
    """update_ref.Net from the last layer's output on: the "observation" is y itself ([M, 1] or [M, 2]),
    so update_ref's passes (cont_pass, choice_pass) run unchanged and grads()[0] is dL/dy per row."""

    def __init__(self, kind, mean=0.0, std=1.0, dtype=torch.float64):
        self.params, self.kind, self.mean, self.std, self.dtype = [], kind, float(mean), float(std), dtype

    def preacts(self, x):
        return [None, None, None, x.to(self.dtype).clone().requires_grad_(True)]

    def grads(self, loss, y):
        g, = torch.autograd.grad(loss, [y])
        return [g.detach()], g.detach().abs().sum(dim=0)


def check(tag, got, g64, g32, K):
    """Print the figures, then assert err <= K * e32 + floor."""
    err = float((torch.from_numpy(got).double() - g64).abs().max())
    e32 = float((g32.double() - g64).abs().max())
    floor = FLOOR * float(g64.abs().max())
    print(f"HEADS {tag} err={err:.4e} e32={e32:.4e} floor={floor:.4e} ratio={err / e32 if e32 > 0 else float('nan'):.3f}")
    assert err <= K * e32 + floor, f"{tag}: err {err:.3e} > {K} * e32 {e32:.3e} + floor {floor:.3e}"


def cont_rows(seed):
    g = torch.Generator().manual_seed(seed)
    M = M_ROWS
    y = (1.2 * torch.randn(M, generator=g)).float()
    mu_old = torch.tanh(y + 0.15 * torch.randn(M, generator=g)) * ic.STD + ic.MEAN
    act = (mu_old + 0.5 ** 0.5 * torch.randn(M, generator=g)).float()
    lp_old = torch.from_numpy(ic.hostfwd().mvn_logp(act.numpy(), mu_old.float().numpy()))
    A = torch.randn(M, generator=g).float()
    return y, act, lp_old, A


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("fd", [0, 1], ids=["f64ratio", "f32ratio"])
def test_cont_row_vs_float64_autograd(fd, seed):
    hf = ic.hostfwd()
    y, act, lp_old, A = cont_rows(seed)
    d = ur.cont_pass(YHead(1, ic.MEAN, ic.STD), y[:, None], act, lp_old, A, float(M_ROWS))["d"]
    keep = ur.away_from_clip(d)
    assert keep.float().mean() >= 0.9
    clipped = ((d < ur.LN_LO) | (d > ur.LN_HI))[keep].float().mean()
    assert 0.05 < clipped < 0.95  # both the followed and the clipped branch of the surrogate are in the batch
    y, act, lp_old, A = y[keep], act[keep], lp_old[keep], A[keep]
    m = float(M_ROWS)
    r64 = ur.cont_pass(YHead(1, ic.MEAN, ic.STD), y[:, None], act, lp_old, A, m)
    r32 = ur.cont_pass(YHead(1, ic.MEAN, ic.STD, torch.float32), y[:, None], act, lp_old, A, m)
    f, dy = hf.cont_row(y.numpy(), ic.MEAN, ic.STD, act.numpy(), lp_old.numpy(), A.numpy(), 1.0 / m, fd)
    check(f"cont fd={fd} seed={seed}", dy, r64["grads"][0][:, 0], r32["grads"][0][:, 0], K_CONT)
    assert abs(f.sum() - float(r64["surr"])) <= 1e-6 * float(r64["surr_abs"])


def choice_rows(seed):
    g = torch.Generator().manual_seed(100 + seed)
    M = M_ROWS
    y = (1.5 * torch.randn(M, 2, generator=g)).float()
    act = (torch.rand(M, generator=g) < 0.35).long()
    y_old = y + 0.2 * torch.randn(M, 2, generator=g)
    lp_old = torch.log_softmax(y_old.double(), -1).gather(1, act[:, None])[:, 0].float()
    A = torch.randn(M, generator=g).float()
    return y, act, lp_old, A


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("mode", ["counts", "per_row"])
def test_choice_row_vs_float64_autograd(mode, seed):
    hf = ic.hostfwd()
    y, act, lp_old, A = choice_rows(seed)
    m = float(M_ROWS)
    counts = ur.action_counts(act)  # of the drawn batch: the global counts (a shard's rows see all M)
    kw = dict(counts=counts) if mode == "counts" else dict(act=act)
    d = ur.choice_pass(YHead(2), y, lp_old, A, m, mode, **kw)["d"]
    keep = ur.away_from_clip(d)
    assert keep.float().mean() >= 0.9
    y, act, lp_old, A = y[keep], act[keep], lp_old[keep], A[keep]
    if mode == "per_row":
        kw = dict(act=act)
        w = torch.zeros(len(act), 2, dtype=torch.float64)
        w[torch.arange(len(act)), act] = m
    else:
        w = counts[None, :].expand(len(act), 2).contiguous()
    r64 = ur.choice_pass(YHead(2), y, lp_old, A, m, mode, **kw)
    r32 = ur.choice_pass(YHead(2, dtype=torch.float32), y, lp_old, A, m, mode, **kw)
    f, dy = hf.choice_row(y.numpy(), lp_old.numpy(), A.numpy(), w.numpy(), 1.0 / (m * m), 1)
    check(f"choice {mode} seed={seed}", dy, r64["grads"][0], r32["grads"][0], K_CHOICE)
    assert abs(f.sum() - float(r64["surr"])) <= 1e-6 * float(r64["surr_abs"])
    if mode == "counts":  # no zero weight: adding every term (k_ppo_choice) is the same sum
        f_all, dy_all = hf.choice_row(y.numpy(), lp_old.numpy(), A.numpy(), w.numpy(), 1.0 / (m * m), 0)
        assert np.array_equal(f_all, f) and np.array_equal(bits32(dy_all), bits32(dy))


def test_choice_term_on_the_clamp_bounds():
    """pn exactly on eps and 1 - eps (the gradient passes, as through torch.clamp), one float32 step
    outside and at 0 and 1 (exactly zero), and inside: the ratio is kept off the clip bounds
    (old = log(clamped pn) - 0.05), so only the clamp can zero the gradient."""
    hf = ic.hostfwd()
    below, above = np.nextafter(EPS32, f32(0)), np.nextafter(EPS32, f32(1))
    hi_in, hi_out = np.nextafter(HI32, f32(0)), np.nextafter(HI32, f32(2))
    pn = np.array([EPS32, HI32, below, hi_out, 0.0, above, hi_in, 0.3, 0.5], np.float32)
    on, outside = slice(0, 2), slice(2, 5)
    A = np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0])
    w, inv_m2 = 7.0, 1.0 / 49.0
    p64 = torch.from_numpy(pn).double().requires_grad_(True)
    lp = torch.log(torch.clamp(p64, ur.EPS, 1.0 - ur.EPS))
    old = (lp - 0.05).detach()
    loss = (w * ur.surrogate(torch.exp(lp - old), torch.from_numpy(A)) * inv_m2).sum()
    g, = torch.autograd.grad(loss, [p64])
    fk, dlp = hf.choice_term(pn, old.numpy(), A, np.full(len(pn), w), inv_m2)
    assert (g[on] != 0).all() and (g[outside] == 0).all()          # what torch.clamp does
    assert np.array_equal(dlp == 0.0, (g == 0).numpy())
    assert np.allclose(dlp, g.numpy(), rtol=1e-6, atol=0.0)
    assert np.allclose(fk, ur.surrogate(torch.exp(lp - old), torch.from_numpy(A)).detach().numpy(), rtol=1e-6)


def test_finish_cont_is_two_roundings_and_softmax_pair_flavours():
    """finish_cont: tanh * std rounded, then + mean rounded (not one fused multiply-add), both flavours;
    softmax_pair: the rollout flavour's bits are test_infer_host.py's; here the special inputs of the
    note in ppo_heads.h (fmaxf against the rollout's former ternary): both results NaN, or equal."""
    hf = ic.hostfwd()
    rng = np.random.default_rng(3)
    z = (2.0 * rng.standard_normal(4000)).astype(np.float32)
    fused_differs = 0
    for update in (0, 1):
        out, t = hf.finish_cont(z, ic.MEAN, ic.STD, update)
        two = t * np.float32(ic.STD) + np.float32(ic.MEAN)
        assert two.dtype == np.float32 and np.array_equal(bits32(out), bits32(two))
        fused = (t.astype(np.float64) * ic.STD + ic.MEAN).astype(np.float32)  # exact product, one rounding
        fused_differs += int((bits32(fused) != bits32(out)).sum())
        assert np.abs(t - np.tanh(z.astype(np.float64))).max() < 3e-7
    assert fused_differs > 100  # the inputs tell the two forms apart
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    zs = np.array([[0.0, -0.0], [-0.0, 0.0], [1.5, 1.5], [nan, 1.0], [1.0, nan], [inf, inf], [-inf, -inf], [inf, 1.0],
                   [-inf, 1.0], [2.0, -3.0]], np.float32)
    for update in (0, 1):
        p = hf.softmax_pair(zs, update)
        mx = np.where(zs[:, 0] > zs[:, 1], zs[:, 0], zs[:, 1])  # the ternary
        with np.errstate(invalid="ignore"):
            e = np.exp((zs - mx[:, None]).astype(np.float64))
            ref = e / e.sum(1, keepdims=True)
        assert np.array_equal(np.isnan(p), np.isnan(ref))
        assert np.array_equal(np.isnan(p[:, 0]), np.isnan(p[:, 1]))
        ok = ~np.isnan(ref)
        assert np.allclose(p[ok], ref[ok], rtol=3e-7, atol=0.0)
        assert np.array_equal(p[:3], np.full((3, 2), 0.5, np.float32)) and np.array_equal(p[8], [0.0, 1.0])
