"""The scalar arithmetic of csrc/ppo_math.h, compiled for the host (tools/hostfwd.cpp hf_*), bit
for bit against torch on the CPU (no GPU): the MVN(loc, 0.5) sample and log-prob and their four
constants against torch.distributions.MultivariateNormal in float32, the clipped surrogate and its
gradient against torch autograd in float64 on a grid that holds the ties, the split-precision
surrogate against the float64 one, and t_minimum against torch.minimum."""
import decimal
import math
import os
import re

import numpy as np
import torch
from torch.distributions import MultivariateNormal

import infer_common as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "mh-ppo_amd", "csrc", "ppo_math.h")).read()
R_MAX = math.sqrt(48.0 * math.log(2.0))  # 5.768: the largest radius of the noise's normals


def constant(name, suffix="f"):
    m = re.search(rf"\b{name} = (-?0x[0-9a-fA-F.]+p[-+]?\d+){suffix}\b", HEADER)
    assert m, name
    return float.fromhex(m.group(1))


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mvn_inputs():
    rng = np.random.default_rng(11)
    n = 100_000
    loc = (3.0 * rng.standard_normal(n) - 1.0).astype(np.float32)
    eps = rng.standard_normal(n).astype(np.float32)
    ext = np.array([0.0, -0.0, R_MAX, -R_MAX], np.float32)
    # the extremes at random locations and at the kernel's start value, and the start value
    # under ordinary noise
    loc = np.concatenate([loc, loc[:4], np.full(4, 2.0, np.float32), np.full(1000, 2.0, np.float32)])
    eps = np.concatenate([eps, ext, ext, eps[:1000]])
    return loc, eps


def test_mvn_sample_and_logp_bits():
    hf = ic.hostfwd()
    loc, eps = mvn_inputs()
    assert loc.size >= 100_000 and loc.dtype == eps.dtype == np.float32
    m = MultivariateNormal(torch.from_numpy(loc)[:, None], covariance_matrix=torch.tensor([[0.5]]))
    e = torch.from_numpy(eps)[:, None]
    a_ref = m.loc + torch.matmul(m.scale_tril, e.unsqueeze(-1)).squeeze(-1)  # rsample's arithmetic
    assert a_ref.dtype == torch.float32 and a_ref.shape == (loc.size, 1)
    a = hf.mvn_sample(loc, eps)
    assert np.array_equal(bits32(a), bits32(a_ref[:, 0].numpy()))
    lp_ref = m.log_prob(a_ref)
    assert lp_ref.dtype == torch.float32 and lp_ref.shape == (loc.size,)
    lp = hf.mvn_logp(a, loc)
    assert np.array_equal(bits32(lp), bits32(lp_ref.numpy()))
    # log-prob of actions that were not sampled from loc (the update's new policy on old actions)
    other = np.roll(loc, 1)
    m2 = MultivariateNormal(torch.from_numpy(other)[:, None], covariance_matrix=torch.tensor([[0.5]]))
    lp2_ref = m2.log_prob(a_ref)
    assert np.array_equal(bits32(hf.mvn_logp(a, other)), bits32(lp2_ref.numpy()))


def test_mvn_constants():
    L = torch.linalg.cholesky(torch.tensor([[0.5]]))
    assert L.dtype == torch.float32
    mvn_l = np.float32(constant("MVN_L"))
    assert mvn_l == L.item() and mvn_l == MultivariateNormal(torch.zeros(1), torch.tensor([[0.5]])).scale_tril.item()
    assert np.float32(constant("MVN_LOG2PI")) == np.float32(math.log(2 * math.pi))
    assert np.float32(constant("MVN_LOG2PI")) == torch.tensor(1 * math.log(2 * math.pi), dtype=torch.float32).item()
    assert np.float32(constant("MVN_HALF_LOGDET")) == torch.log(L).item()
    # 1/L: float32(1 / L), what a triangular solve against [[L]] multiplies by, and the factor
    # with which log_prob's bits match (test_mvn_sample_and_logp_bits); its float32 neighbours
    # do not reproduce log_prob
    inv = np.float32(constant("MVN_INV_L"))
    assert inv == np.float32(1.0) / mvn_l
    assert inv == torch.linalg.solve_triangular(L, torch.ones(1, 1), upper=False).item()
    loc, eps = mvn_inputs()
    a = ic.hostfwd().mvn_sample(loc, eps)
    lp_ref = MultivariateNormal(torch.from_numpy(loc)[:, None], covariance_matrix=torch.tensor([[0.5]])).log_prob(
        torch.from_numpy(a)[:, None]).numpy()

    def logp_with(inv_l):
        x = (a - loc) * inv_l
        return np.float32(-0.5) * (np.float32(constant("MVN_LOG2PI")) + x * x) - np.float32(constant("MVN_HALF_LOGDET"))

    assert np.array_equal(bits32(logp_with(inv)), bits32(lp_ref))
    for wrong in (np.nextafter(inv, np.float32(0)), np.nextafter(inv, np.float32(2))):
        share = (bits32(logp_with(wrong)) != bits32(lp_ref)).mean()
        print(f"1/L = {float(wrong)!r}: {100 * share:.1f} % of log-probs differ")
        assert share > 0.01


# ---------------------------------------------------------------- the clipped surrogate
def surr_grid():
    rng = np.random.default_rng(5)
    r = [0.0, 0.5, 0.8, np.nextafter(0.8, 0.0), np.nextafter(0.8, 1.0), 1.0, 1.2, np.nextafter(1.2, 0.0),
         np.nextafter(1.2, 2.0), 1.7, 1e300]
    r = np.concatenate([r, np.exp(rng.normal(0.0, 0.3, 3000))])
    A = np.concatenate([[2.5, -2.5, 0.0, -0.0, 1e-300, 3.25], rng.standard_normal(20), 5.0 * rng.standard_normal(5)])
    rr, AA = np.meshgrid(r, A, indexing="ij")
    return rr.ravel(), AA.ravel()


def test_surr_and_grad_vs_autograd():
    """-min(r A, clamp(r, 0.8, 1.2) A) and d/dr from torch autograd in float64: torch.min splits
    the gradient evenly between equal terms, and clamp passes it on [0.8, 1.2] inclusive.  Values
    and gradients bit for bit (np.array_equal: equal float64 values have equal bits, except zeros
    of either sign, which compare by value)."""
    hf = ic.hostfwd()
    r, A = surr_grid()
    rt = torch.tensor(r, requires_grad=True)
    At = torch.tensor(A)
    assert rt.dtype == torch.float64
    f_ref = -torch.min(rt * At, torch.clamp(rt, 0.8, 1.2) * At)
    f_ref.sum().backward()
    f, g = hf.surr_and_grad(r, A)
    assert np.isfinite(f_ref.detach().numpy()).all()
    assert np.array_equal(f, f_ref.detach().numpy())
    assert np.array_equal(g, rt.grad.numpy())
    # the rule itself, on torch's gradient: -A on [0.8, 1.2] inclusive (both terms tie and clamp
    # passes the gradient: 0.5 A + 0.5 A); below, -A for A > 0 and 0 for A < 0; above, the reverse
    gn = rt.grad.numpy()
    inside, below, above = (r >= 0.8) & (r <= 1.2), r < 0.8, r > 1.2
    assert ((r == 0.8).sum() > 0) and ((r == 1.2).sum() > 0) and below.sum() > 100 and above.sum() > 100
    assert np.array_equal(gn[inside], -A[inside])
    # one float64 step outside the bounds the two products can still round to the same number:
    # minimum splits the gradient, clamp passes none: -0.5 A (the grid holds such rows)
    rounded_tie = ~inside & (r * A == np.clip(r, 0.8, 1.2) * A) & (A != 0)
    assert rounded_tie.any() and np.array_equal(gn[rounded_tie], -0.5 * A[rounded_tie])
    rest = (below | above) & ~rounded_tie
    assert np.array_equal(gn[rest], np.where((A > 0) == below, -A, 0.0 * A)[rest])


def exp_rounded(d):
    """The correctly rounded float64 exp(d), from 60-digit arithmetic."""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        return float(decimal.Decimal(float(d)).exp())


def steps(x, k):
    """The double k steps from x."""
    for _ in range(abs(k)):
        x = np.nextafter(x, math.inf if k > 0 else -math.inf)
    return float(x)


def test_clip_thresholds():
    """LN_0_8 is the smallest double whose correctly rounded exp is >= 0.8, LN_1_2 the largest whose
    exp is <= 1.2 (exp(d) equals the bound, a tie that clamp passes, for a few doubles around the
    rounded logarithms), so `d < LN_0_8` is `exp(d) < 0.8` for every double d."""
    lo, hi = constant("LN_0_8", suffix=""), constant("LN_1_2", suffix="")
    assert exp_rounded(lo) == 0.8 and exp_rounded(steps(lo, -1)) == np.nextafter(0.8, 0.0)
    assert exp_rounded(hi) == 1.2 and exp_rounded(steps(hi, 1)) == np.nextafter(1.2, 2.0)
    assert steps(lo, 2) == math.log(0.8) and steps(hi, -3) == math.log(1.2)
    assert (ic.LN_0_8, ic.LN_1_2) == (lo, hi)  # the tests' copy


def fd_inputs():
    """d, the float64 ratio exp(d), A.  Around the thresholds the ratio is the correctly rounded one
    (numpy's and the C library's exp differ from each other there, by one step)."""
    rng = np.random.default_rng(6)
    near = []
    for c in (math.log(0.8), math.log(1.2)):
        near += [steps(c, k) for k in range(-5, 6)]  # holds both neighbours of LN_0_8 and of LN_1_2
        q = math.floor(c * 2.0**24)
        near += [(q - 1) * 2.0**-24, q * 2.0**-24, (q + 1) * 2.0**-24, (q + 2) * 2.0**-24]  # the log-densities' grid
    for c in (constant("LN_0_8", suffix=""), constant("LN_1_2", suffix="")):
        assert steps(c, -1) in near and steps(c, 1) in near
    rand = np.concatenate([rng.normal(0.0, 0.3, 4000), np.round(rng.normal(0.0, 0.3, 4000) * 2.0**24) * 2.0**-24])
    assert min(np.abs(rand - math.log(0.8)).min(), np.abs(rand - math.log(1.2)).min()) > 1e-12
    d = np.concatenate([near, rand])
    r = np.concatenate([[exp_rounded(x) for x in near], np.exp(rand)])
    A = np.concatenate([[2.5, -2.5, 0.0, -0.0, 3.25], rng.standard_normal(12)]).astype(np.float32)
    i, j = [x.ravel() for x in np.meshgrid(np.arange(d.size), np.arange(A.size), indexing="ij")]
    return d[i], r[i], A[j]


def test_surr_and_grad_fd_vs_float64():
    """The split-precision surrogate (float32 ratio, branch from the float64 d = lp - lp_old)
    against surr_and_grad(exp(d), A) in float64: the gradient takes the same branch (-A or 0, by
    value), and the value is the one float32 rounding of r A (r the float32 ratio) where the
    reference follows r, of 0.8f A resp. 1.2f A where it is clipped."""
    hf = ic.hostfwd()
    d, r64, A = fd_inputs()
    r32 = r64.astype(np.float32)
    A64 = A.astype(np.float64)
    f64, g64 = hf.surr_and_grad(r64, A64)
    f, g = hf.surr_and_grad_fd(r32, d, A)
    assert f.dtype == g.dtype == np.float32
    # One float64 step outside a bound the reference's two float64 products can round to the same
    # number, and torch's minimum then halves the gradient (test_surr_and_grad_vs_autograd).  The
    # split-precision form has no float64 product: there it gives the gradient of a ratio outside
    # the bounds.  Such rows exist here only next to the thresholds, and are asserted as that.
    outside = (r64 < 0.8) | (r64 > 1.2)
    halved = outside & (A64 != 0) & (r64 * A64 == np.clip(r64, 0.8, 1.2) * A64)
    assert halved.any() and np.array_equal(g64[halved], -0.5 * A64[halved])
    assert np.abs(r64[halved] / np.round(r64[halved], 1) - 1.0).max() < 1e-15
    g64 = np.where(halved, np.where((A64 > 0) == (r64 < 0.8), -A64, 0.0), g64)
    assert np.all((g64 == -A64) | (g64 == 0.0))
    assert np.array_equal(g.astype(np.float64), g64)
    follows = f64 == -(r64 * A64)  # the reference's value is the unclipped term (or both tie)
    rc = np.where(r64 < 1.0, np.float32(0.8), np.float32(1.2)).astype(np.float64)
    want = -np.where(follows, r32.astype(np.float64) * A64, rc * A64)  # exact: 24 x 24 bits
    assert np.array_equal(f, want.astype(np.float32))
    for bound in (0.8, 1.2):  # below, at and above each bound, with both signs of A
        for side in (r64 < bound, r64 == bound, r64 > bound):
            assert (side & (A64 > 0) & (np.abs(r64 - bound) < 1e-15)).any()
            assert (side & (A64 < 0) & (np.abs(r64 - bound) < 1e-15)).any()
    assert follows.any() and (~follows).any() and (g64[A64 != 0] == 0).any()


# ---------------------------------------------------------------- torch.minimum
def test_t_minimum_vs_torch_minimum():
    """t_minimum against torch.minimum in float32, one element at a time (torch's scalar path) and
    on arrays of >= 64 (its vector path): bit for bit, a NaN in either slot giving a NaN.  Where
    torch's two paths disagree with each other on the sign of a zero tie (min(+0, -0)), that case is
    compared by value: the sign of a zero cannot reach the rollout, whose `out == loc` test and
    arithmetic treat both zeros alike."""
    hf = ic.hostfwd()
    rng = np.random.default_rng(9)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    special = np.array([0.0, -0.0, 1.0, -1.0, 2.0, nan, inf, -inf, 1e-45, -1e-45], np.float32)
    a, b = [x.ravel() for x in np.meshgrid(special, special, indexing="ij")]
    x = rng.standard_normal(200).astype(np.float32)
    a = np.concatenate([a, x, x])
    b = np.concatenate([b, np.roll(x, 3), x])
    assert a.size >= 64
    got = hf.t_minimum(a, b)
    vec = torch.minimum(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    one = np.array([torch.minimum(torch.from_numpy(a[i:i + 1]), torch.from_numpy(b[i:i + 1])).item()
                    for i in range(a.size)], np.float32)
    isnan = np.isnan(a) | np.isnan(b)
    zero_tie = (a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))
    assert zero_tie.sum() == 2 and isnan.sum() == 19
    paths_differ = bits32(vec) != bits32(one)
    print(f"torch.minimum: scalar and vector paths differ in {int((paths_differ & ~isnan).sum())} non-NaN cases "
          f"(zero ties: {int((paths_differ & zero_tie).sum())})")
    assert not (paths_differ & ~isnan & ~zero_tie).any()
    for ref in (vec, one):
        assert np.array_equal(np.isnan(got), isnan) and np.array_equal(np.isnan(ref), isnan)
        exact = ~isnan & ~(zero_tie & paths_differ)
        assert np.array_equal(bits32(got)[exact], bits32(ref)[exact])
        assert np.all(got[zero_tie] == 0.0) and np.all(ref[zero_tie] == 0.0)
