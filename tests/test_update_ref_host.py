"""tests/update_ref.py (the float64 reference the train-kernel tests compare against) proved on the
CPU: its literal M x M choice loss against its O(M) count-weighted form, its epoch-0 losses against
the reference program's recorded ones (tests/golden/ppo_update.npz), and the surrogate's gradient
at its ties and edges against the rule csrc/ppo_math.h states for torch."""
import os

import numpy as np
import pytest
import torch

import update_ref as ur

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "ppo_update.npz")
LAYERS = [f"layer{i}.{w}" for i in (1, 2, 3, 4) for w in ("weight", "bias")]


def _rand_net(gen, n_in, n_out, kind, scale4=1.0):
    ps = []
    for shp in ur.param_shapes(n_in, n_out):
        fan_in = shp[1] if len(shp) == 2 else {32: n_in, 64: 32}.get(shp[0], 32)
        ps.append((torch.rand(shp, generator=gen, dtype=torch.float64) * 2 - 1) / fan_in ** 0.5)
    ps[6], ps[7] = ps[6] * scale4, ps[7] * scale4
    return ur.Net(ps, kind)


@pytest.mark.parametrize("scale4", [1.0, 300.0], ids=["init", "saturated"])
def test_literal_choice_loss_equals_count_weighted_form(scale4):
    """The M x M Categorical broadcast, written out, against sum_j sum_k n_k f(r_jk, A_j): loss and
    every gradient tensor to 1e-12 relative, M = 257, random actions (so random counts); also with a
    scaled output layer, where part of the rows sit on the clamp of the probabilities."""
    gen = torch.Generator().manual_seed(5)
    M, dc = 257, 27
    net = _rand_net(gen, dc, 2, 2, scale4)
    obs = torch.randn(M, dc, generator=gen, dtype=torch.float64) * 2
    act = (torch.rand(M, generator=gen) < 0.37).double()
    lpo = torch.log(torch.rand(M, generator=gen, dtype=torch.float64) * 0.8 + 0.1)
    A = torch.randn(M, generator=gen, dtype=torch.float64)
    counts = ur.action_counts(act)
    assert counts.min() > 0 and float(counts.sum()) == M
    lit = ur.choice_pass(net, obs, lpo, A, float(M), "literal", act=act)
    cnt = ur.choice_pass(net, obs, lpo, A, float(M), "counts", counts=counts)
    if scale4 > 1:
        pn = net(obs).detach()
        clamped = ((pn < ur.EPS) | (pn > 1 - ur.EPS)).any(dim=1).double().mean()
        assert 0.1 < float(clamped) < 0.9, float(clamped)
    assert abs(float(lit["surr"] - cnt["surr"])) <= 1e-12 * abs(float(cnt["surr"]))
    for name, gl, gc in zip(ur.PARAM_NAMES, lit["grads"], cnt["grads"]):
        assert float(gc.abs().max()) > 0, name
        assert float((gl - gc).abs().max()) <= 1e-12 * float(gc.abs().max()), name


def _golden_net(g, head, which, kind, mean=0.0, std=1.0):
    return ur.Net([torch.tensor(g[f"{head}_init_{which}_{k}"]) for k in LAYERS], kind, mean, std)


@pytest.mark.parametrize("head", ["c", "d"])
def test_epoch0_losses_match_the_reference_programs(head):
    """On the init weights of the golden run, both heads: the reference program's own epoch-0 actor
    and critic losses, at the 1e-4 relative test_update_matches_reference uses for them."""
    g = np.load(G)
    obs, ret = torch.tensor(g[f"{head}_obs"]), torch.tensor(g[f"{head}_rtgs"])
    lpo = torch.tensor(g[f"{head}_logp"])
    act = torch.tensor(g[f"{head}_act"]).double()
    M = obs.shape[0]
    m = float(M)
    critic = _golden_net(g, head, "critic", 0)
    c = ur.critic_pass(critic, obs, ret, m)
    A = ur.advantage(ret, c["V"], torch.stack([c["sum_a"], c["sum_a2"]]), m)
    assert abs(float(A.mean())) < 1e-9 and abs(float(A.std()) - 1) < 1e-9  # torch's own normalisation
    if head == "c":
        a = ur.cont_pass(_golden_net(g, head, "actor", 1, -1.0, 3.0), obs, act, lpo, A, m)
        la = float(a["surr"]) / m
    else:
        assert M <= ur.LITERAL_MAX_ROWS
        a = ur.choice_pass(_golden_net(g, head, "actor", 2), obs, lpo, A, m, "literal", act=act)
        la = float(a["surr"]) / (m * m)
    lc = float(c["sse"]) / m
    ref_a, ref_c = g[f"{head}_losses"][0]
    assert abs(la - ref_a) <= 1e-4 * abs(ref_a), (la, ref_a)
    assert abs(lc - ref_c) <= 1e-4 * abs(ref_c), (lc, ref_c)


# (r, A, d/dr of -min(r A, clamp(r, .8, 1.2) A)) as csrc/ppo_math.h states torch's rule: minimum
# splits the gradient evenly on a tie, clamp passes it on [0.8, 1.2] inclusive.  With s1 = r A,
# s2 = clamp(r) A: s1 < s2 -> -A; s2 < s1 -> -(in A); tie -> -(A/2 + in A/2); in = 1 on [0.8, 1.2].
EDGES = [
    (0.8, 2.0, -2.0), (0.8, -2.0, 2.0),      # r exactly 0.8: tie, clamp passes
    (1.2, 2.0, -2.0), (1.2, -2.0, 2.0),      # r exactly 1.2: tie, clamp passes
    (1.0, 2.0, -2.0), (1.0, -2.0, 2.0),      # in between: tie of equal terms
    (0.95, 0.5, -0.5), (1.1, -0.5, 0.5),
    (0.5, 2.0, -2.0), (0.5, -2.0, 0.0),      # below: follows r for A > 0, constant for A < 0
    (1.5, 2.0, 0.0), (1.5, -2.0, 2.0),       # above: constant for A > 0, follows r for A < 0
    (0.8, 0.0, 0.0), (1.2, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 0.0, 0.0), (1.5, 0.0, 0.0),  # A = 0
]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_surrogate_gradient_at_ties_and_edges(dtype):
    r = torch.tensor([e[0] for e in EDGES], dtype=dtype, requires_grad=True)
    A = torch.tensor([e[1] for e in EDGES], dtype=dtype)
    want = torch.tensor([e[2] for e in EDGES], dtype=dtype)
    f = ur.surrogate(r, A)
    (g,) = torch.autograd.grad(f.sum(), r)
    assert torch.equal(g, want), (g, want)
    rc = r.detach().clamp(0.8, 1.2)
    assert torch.equal(f.detach(), -torch.minimum(r.detach() * A, rc * A))


def test_per_row_mode_is_the_literal_diagonal():
    """The per-row surrogate (sum_j f(r_j a_j, A_j) / m) is the diagonal i = j of the literal tensor
    over m: the literal form with one row at a time, summed, times 1 / m instead of 1 / m^2."""
    gen = torch.Generator().manual_seed(9)
    M, dc = 37, 12
    net = _rand_net(gen, dc, 2, 2)
    obs = torch.randn(M, dc, generator=gen, dtype=torch.float64) * 2
    act = (torch.rand(M, generator=gen) < 0.5).double()
    lpo = torch.log(torch.rand(M, generator=gen, dtype=torch.float64) * 0.8 + 0.1)
    A = torch.randn(M, generator=gen, dtype=torch.float64)
    pr = ur.choice_pass(net, obs, lpo, A, float(M), "per_row", act=act)
    tot, gs = 0.0, None
    for j in range(M):
        one = ur.choice_pass(net, obs[j:j + 1], lpo[j:j + 1], A[j:j + 1], 1.0, "literal", act=act[j:j + 1])
        tot += float(one["surr"])
        gs = one["grads"] if gs is None else [a + b for a, b in zip(gs, one["grads"])]
    assert abs(tot * M - float(pr["surr"])) <= 1e-12 * abs(float(pr["surr"]))
    for name, a, b in zip(ur.PARAM_NAMES, gs, pr["grads"]):
        assert float((a / M - b).abs().max()) <= 1e-12 * float(b.abs().max()), name


def test_cont_logp_is_the_multivariate_normal():
    """cont_logp against MultivariateNormal(mu, [[0.5]]).log_prob as the reference program calls it."""
    gen = torch.Generator().manual_seed(3)
    net = _rand_net(gen, 13, 1, 1)
    net.mean, net.std = -1.0, 3.0
    obs = torch.randn(50, 13, generator=gen, dtype=torch.float64) * 3
    act = torch.randn(50, generator=gen, dtype=torch.float64) - 1
    cov = torch.diag(torch.full(size=(1,), fill_value=0.5, dtype=torch.float64))
    with torch.no_grad():
        want = torch.distributions.MultivariateNormal(net(obs)[:, None], cov).log_prob(act[:, None])
        got = ur.cont_logp(net, obs, act)
    assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())


def test_split_packed_round_trip():
    flat = torch.arange(32 * 5 + 32 + 2048 + 64 + 2048 + 32 + 64 + 2, dtype=torch.float32)
    parts = ur.split_packed(flat, 5, 2)
    assert [tuple(p.shape) for p in parts] == ur.param_shapes(5, 2)
    assert torch.equal(torch.cat([p.reshape(-1) for p in parts]), flat)
    with pytest.raises(ValueError):
        ur.split_packed(flat[:-1], 5, 2)
