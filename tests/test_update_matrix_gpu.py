"""Every instantiation of the fused update kernels (mhppo_mlp_train, mhppo_mlp_train_pair) at the row
counts its launch geometry makes special, against tests/update_ref.py: a float64 torch autograd of
the same pass on the same weights and batch (proved on the CPU by test_update_ref_host.py).

Which parameter set reaches which kernel entry (csrc/mlp_train.hip), all at row counts below 200
(1, 31, 32, 33, 32 W - 1, 32 W, 32 W + 1) and the marked ones also at 32 W C + 33 and 4 * 32 W C + 33
(W waves per block, C compute units: one wave takes a second tile, so the prefetch path runs once;
one wave takes five tiles, so the four LDS image slots wrap):
  x3_kernel (family "x3", exact=False, W = 4)
    <K_CRITIC, G13S>, <K_CONT, G13S>        x3-c13 *   (and the critic of x3-d13)
    <K_CRITIC, GV16>, <K_CHOICE, GC16>      x3-d1, x3-d13 (actor only), x3-d15 *
    <K_CRITIC, GV32>, <K_CHOICE, GC32>      x3-d16, x3-d31 *
    <K_CRITIC, GV64>, <K_CHOICE, GC64>      x3-d32, x3-d53 *
    <K_CRITIC, GV54>, <K_CHOICE, GC54>      x3-d54 *
  f32_launcher (family "f32": exact=True; family "auto": exact=False above 54 inputs; W = 4, the
  13-input ones W = 8)
    launch<K_CRITIC / K_CONT, 7, true>      f32-c13 *
    launch<K_CRITIC / K_CHOICE, 8, false>   f32-d1, f32-d16 *
    launch<.., 12, false>                   f32-d17, f32-d24 *
    launch<.., 16, false>                   f32-d25, f32-d32 *
    launch<.., 24, false>                   f32-d33, f32-d48 *
    launch<.., 28, false>                   f32-d49, f32-d56 *, auto-d55 *
    launch<.., 32, false>                   f32-d57, f32-d64 *, auto-d64
  k_mlp_train_x3_pair                       test_pair_* (every row count above)
Every choice cell runs the actor in both modes: the global action counts, and per row with `act`.

Compared per cell: V, the three float64 sums, and the gradient tensor by tensor (W1, b1, .., W4, b4).
Bound per tensor t:  ek_t <= K * e32_t + floor_t, with ek_t the kernel's max-abs error against
float64, e32_t that of torch's own float32 autograd of the same loss on the same GPU, and floor_t =
4 float32 ulps (4 * 2^-23) of max|g64_t| for the cells where torch happens to be (nearly) exact.  V: the
same against torch's float32 forward.  Two tensors hold one or two numbers that are sums which
cancel, and a few ulps of a cancelled sum is not what float32 arithmetic delivers (the issue is the
one the advantage sum has, whose bar is taken of sum|A|): b4's gradient, the plain sum over rows of
dL/dy (the choice head's rows pull the logit pair both ways; at M = 33 the sum was seen 30 times
smaller than its terms' magnitudes), takes its floor of sum_rows |dL/dy|, and V, one dot product
per row (one number at M = 1), of the largest row's sum_k |W4_k h3_k| + |b4|.
Sums: 1e-6 relative, the advantage sum (which cancels) within 1e-6 of sum|A| and the surrogate's
within 1e-6 of the sum of its terms' magnitudes (the bars of test_update_scale_gpu.py).  The choice actor's float64 reference is the literal M x M broadcast
up to 1 024 rows and its O(M) form above; torch's float32 yardstick is always the O(M) form (its
gradient needs no 1 024-way scatter-add, so the yardstick is the tighter one).

K is twice the worst ek_t / e32_t measured over this whole file on an MI355X (the factor 2: the
kernels' summation trees legitimately differ from torch's, both limited by float32 rounding),
per kernel family.  The ratio is taken over the cells with e32_t above floor_t (below it the floor
decides).  Measured worst ratios per tensor:
                       V     W1    b1    W2    b2    W3    b3    W4    b4
  bf16x3  critic     1.37  0.06    -   0.06    -   0.05    -   0.06    -
          cont         -   1.15  1.74  1.34  1.42  1.38  1.69  1.35  1.34
          choice       -   1.99  2.18  2.53  2.22  2.26  2.35  2.51  2.35    worst 2.53, K = 5.1
  f32     critic     1.00  0.05    -   0.07    -   0.05    -   0.07    -
          cont         -   1.00  1.74  1.15  1.49  1.18  1.80  2.74  0.90
          choice       -   1.66  1.70  1.79  1.79  1.90  1.79  1.82  1.79    worst 2.74, K = 5.5
(-: torch's error never rose above the floor.  The critic's weight gradients are ~16 times closer to
float64 than torch's: the kernels fold their per-wave partials in float64.)  bf16x3 covers the split
kernel and the pair kernel, f32 the exact kernel asked for (exact=True) and taken above 54 inputs.
With one of the six bf16 products removed from the split kernel's product primitive (mfma6, the
mid x mid term, 2^-16 per product) 63 of the 64 x3-d* cells of test_instantiation_at_row_count fail
even with K = 16, worst ratio 57.7, while all 16 cases of test_fused_choice_grads_vs_autograd (1e-4 of the packed
gradient's max) still pass on that build.

Batches: the float64 forward alone decides which rows a batch holds, before any kernel runs
(update_ref.away_from_kinks / away_from_clip: a row within 1e-4 of a ReLU kink or of a clip bound
may legitimately take the other branch in float32, torch's as much as the kernels'; the regime
tests below add their bands).  About twice the rows are drawn, filtered, then cut to M.

Not tested: constant returns (ret - V equal on all rows up to float32 rounding).  The advantage's
normalisation is then degenerate (a variance that is all rounding error divided by itself), in the
reference program as much as here.
"""
import pytest
import torch

import update_ref as ur

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")

# twice the worst measured ek_t / e32_t of the family (module docstring)
K_BOUND = {"bf16x3": 5.1, "f32": 5.5}
FLOOR = 4 * 2.0 ** -23
FAMILY = {"x3": "bf16x3", "pair": "bf16x3", "f32": "f32", "auto": "f32"}

SMALL = ("1", "31", "32", "33", "blk-1", "blk", "blk+1")
LARGE = ("grid+33", "4grid+33")
CONFIGS = ([("x3", "c", 13)] + [("x3", "d", n) for n in (1, 13, 15, 16, 31, 32, 53, 54)] + [("f32", "c", 13)] +
           [("f32", "d", n) for n in (1, 16, 17, 24, 25, 32, 33, 48, 49, 56, 57, 64)] +
           [("auto", "d", 55), ("auto", "d", 64)])
# one n_in per kernel entry also runs the two large row counts
WITH_LARGE = {("x3", "c", 13), ("x3", "d", 15), ("x3", "d", 31), ("x3", "d", 53), ("x3", "d", 54), ("f32", "c", 13),
              ("f32", "d", 16), ("f32", "d", 24), ("f32", "d", 32), ("f32", "d", 48), ("f32", "d", 56),
              ("f32", "d", 64), ("auto", "d", 55)}
CELLS = [pytest.param(f, h, n, t, id=f"{f}-{h}{n}-M{t}")
         for (f, h, n) in CONFIGS for t in SMALL + (LARGE if (f, h, n) in WITH_LARGE else ())]


def _waves(fam, head, n_in):
    """Waves per block of the cell's launches (mhppo_mlp_train): 4 on the split kernel, 8 on the
    13-input exact kernel, 4 on the other exact ones."""
    return 8 if (fam != "x3" and head == "c" and n_in == 13) else 4


def _rows(tag, W):
    C = torch.cuda.get_device_properties(0).multi_processor_count
    return {"1": 1, "31": 31, "32": 32, "33": 33, "blk-1": 32 * W - 1, "blk": 32 * W, "blk+1": 32 * W + 1,
            "grid+33": 32 * W * C + 33, "4grid+33": 4 * 32 * W * C + 33}[tag]


class _Batch:
    pass


def _make(head, n_in, M, seed, xs, scale4=1.0, band=None, deltas=None, net_seed=None):
    """Default-init nets (layer 4 of the actor scaled by scale4) and a batch of M rows on the GPU, the
    rows chosen by the float64 forward alone: away from ReLU kinks and clip bounds, outside `band`
    (of |y| for the continuous actor, of the logit gap |y0 - y1| for the choice actor).  deltas: set
    logp_old = float32(logp64 - d), d drawn from deltas, logp64 the row's own action's.  net_seed: the
    nets' initialisation seed when it is not the batch's (the regime tests fix the nets per input width)."""
    from mhppo.models import Model_PPO
    torch.manual_seed(seed if net_seed is None else net_seed)
    actor = Model_PPO(13, 1, 1, mean=-1.0, std=3.0) if head == "c" else Model_PPO(n_in, 2, 2)
    critic = Model_PPO(n_in, 1, 0)
    if scale4 != 1.0:
        with torch.no_grad():
            actor.layer4.weight.mul_(scale4)
            actor.layer4.bias.mul_(scale4)
    actor, critic = actor.to(DEV), critic.to(DEV)
    gen = torch.Generator().manual_seed(seed + 1)
    n = 2 * M + 64
    obs = (torch.randn(n, n_in, generator=gen) * xs).to(DEV)
    if head == "c":
        ret = (torch.randn(n, generator=gen) * 8 - 20).to(DEV)
        act = (torch.randn(n, generator=gen) - 1).to(DEV)
        lpo = (torch.randn(n, generator=gen) * 0.3 - 0.9).to(DEV)
    else:
        ret = (torch.randn(n, generator=gen) * 3 - 5).to(DEV)
        act = (torch.rand(n, generator=gen) < 0.4).float().to(DEV)
        lpo = torch.log(torch.rand(n, generator=gen) * 0.8 + 0.1).to(DEV)
    b = _Batch()
    b.a64, b.c64 = ur.Net.of(actor), ur.Net.of(critic)
    with torch.no_grad():
        keep = ur.away_from_kinks([b.a64, b.c64], obs)
        y = b.a64.preacts(obs)[3]
        if head == "c":
            lp64 = ur.cont_logp(b.a64, obs, act)
            gap = y[:, 0].abs()
        else:
            logits = ur.choice_logits(b.a64, obs)
            lp64 = logits.gather(1, act.long()[:, None])[:, 0]
            gap = (y[:, 0] - y[:, 1]).abs()
        if deltas is not None:
            pick = torch.randint(len(deltas), (n,), generator=gen)
            lpo = (lp64 - torch.tensor(deltas, dtype=torch.float64)[pick].to(DEV)).float()
        d = (lp64 - lpo.double()) if head == "c" else (logits - lpo.double()[:, None])
        keep &= ur.away_from_clip(d)
        if band is not None:
            keep &= ~((gap >= band[0]) & (gap <= band[1]))
    idx = keep.nonzero()[:, 0][:M]
    assert idx.numel() == M, f"{int(keep.sum())} of {n} rows kept, {M} needed"
    b.actor, b.critic, b.head, b.n_in, b.M = actor, critic, head, n_in, M
    b.obs, b.ret, b.act, b.lpo, b.gap = (t[idx].contiguous() for t in (obs, ret, act, lpo, gap))
    b.m = float(M) if M > 1 else 2.0  # the unbiased std needs m > 1
    return b


def _cmp(bad, tag, fam, name, got, r64, r32, scale=None):
    """Print the figures of one tensor, then note it in `bad` if ek > K e32 + floor (floor: FLOOR
    times `scale`, by default max|r64|)."""
    ek = float((got.double() - r64).abs().max())
    e32 = float((r32.double() - r64).abs().max())
    floor = FLOOR * float(r64.abs().max() if scale is None else scale)
    K = K_BOUND[FAMILY[fam]]
    print(f"UPDM {FAMILY[fam]} {tag} {name} ek={ek:.4e} e32={e32:.4e} floor={floor:.4e}")
    if not ek <= K * e32 + floor:
        bad.append(f"{tag} {name}: ek {ek:.3e} > {K} * e32 {e32:.3e} + floor {floor:.3e}")


def _cmp_grads(bad, tag, fam, what, flat, r64, r32, n_in, n_out):
    for name, gk, a, c in zip(ur.PARAM_NAMES, ur.split_packed(flat, n_in, n_out), r64["grads"], r32["grads"]):
        # b4's gradient is the plain sum over rows of dL/dy, one or two numbers, and it cancels (the
        # choice head's rows pull the logit pair both ways): its floor is taken of the sum of the rows'
        # magnitudes, as the advantage sum's bar is taken of sum|A|
        _cmp(bad, tag, fam, f"{what}.{name}", gk, a, c, r64["dy_abs"].max() if name == "b4" else None)


def _rel(bad, tag, name, got, want, scale):
    got, want, scale = float(got), float(want), float(scale)
    print(f"UPDM sum {tag} {name} got={got!r} want={want!r} err/scale={abs(got - want) / scale if scale else 0.0:.3e}")
    if not abs(got - want) <= 1e-6 * scale:
        bad.append(f"{tag} {name}: {got!r} vs {want!r}, 1e-6 of {scale!r}")


def _check_critic(bad, tag, fam, b, got):
    """got = (grad, sums, V) of a critic pass on b.critic's present weights."""
    gc, sc, V = got
    r64 = ur.critic_pass(ur.Net.of(b.critic), b.obs, b.ret, b.m)
    r32 = ur.critic_pass(ur.Net.of(b.critic, torch.float32), b.obs, b.ret, b.m)
    # V is one dot product per row, which cancels: its floor is taken of the terms' magnitudes
    _cmp(bad, tag, fam, "critic.V", V, r64["V"], r32["V"], r64["v_terms"])
    _cmp_grads(bad, tag, fam, "critic", gc, r64, r32, b.n_in, 1)
    _rel(bad, tag, "critic.sse", sc[0], r64["sse"], r64["sse"])
    _rel(bad, tag, "critic.sum_a", sc[1], r64["sum_a"], r64["sum_abs_a"])
    _rel(bad, tag, "critic.sum_a2", sc[2], r64["sum_a2"], r64["sum_a2"])


def _actor_refs(b, V, stats, mode):
    """(float64, float32) reference passes of the actor for the V and advantage sums the kernel gets."""
    out = []
    for dt in (torch.float64, torch.float32):
        net = ur.Net.of(b.actor, dt)
        A = ur.advantage(b.ret, V, stats, b.m, dt)
        if b.head == "c":
            out.append(ur.cont_pass(net, b.obs, b.act, b.lpo, A, b.m))
        elif mode == "per_row":
            out.append(ur.choice_pass(net, b.obs, b.lpo, A, b.m, "per_row", act=b.act))
        else:
            lit = dt == torch.float64 and b.M <= ur.LITERAL_MAX_ROWS
            out.append(ur.choice_pass(net, b.obs, b.lpo, A, b.m, "literal" if lit else "counts", act=b.act,
                                      counts=ur.action_counts(b.act)))
    return out


def _check_actor(bad, tag, fam, b, got, V, stats, mode):
    ga, sa = got
    r64, r32 = _actor_refs(b, V, stats, mode)
    what = "cont" if b.head == "c" else f"choice[{mode}]"
    _cmp_grads(bad, tag, fam, what, ga, r64, r32, b.n_in, 1 if b.head == "c" else 2)
    _rel(bad, tag, f"{what}.surr", sa[0], r64["surr"], r64["surr_abs"])
    if float(sa[1]) != 0.0 or float(sa[2]) != 0.0:
        bad.append(f"{tag} {what}: sums[1:3] = {sa[1:].tolist()}, not 0")
    return r64


def _actor_pass(b, V, stats, mode, exact):
    from mhppo import ppo
    if b.head == "c":
        ga, sa, _ = ppo.k_mlp_train(ppo.KIND_CONT, b.actor, b.obs, b.ret, V, b.act, b.lpo, stats, m_global=b.m,
                                    exact=exact)
    elif mode == "per_row":
        ga, sa, _ = ppo.k_mlp_train(ppo.KIND_CHOICE, b.actor, b.obs, b.ret, V, b.act, b.lpo, stats, None,
                                    m_global=b.m, exact=exact)
    else:
        ga, sa, _ = ppo.k_mlp_train(ppo.KIND_CHOICE, b.actor, b.obs, b.ret, V, None, b.lpo, stats,
                                    ur.action_counts(b.act), m_global=b.m, exact=exact)
    return ga.clone(), sa.clone()


def _run_cell(bad, tag, fam, b):
    """The critic pass and the actor pass(es) of one head on one batch against the references."""
    from mhppo import ppo
    exact = fam == "f32"
    gc, sc, V = ppo.k_mlp_train(ppo.KIND_CRITIC, b.critic, b.obs, b.ret, m_global=b.m, exact=exact)
    _check_critic(bad, tag, fam, b, (gc.clone(), sc.clone(), V))
    stats = ur.adv_sums(b.ret, V)
    out = {}
    for mode in (("cont",) if b.head == "c" else ("counts", "per_row")):
        out[mode] = _check_actor(bad, tag, fam, b, _actor_pass(b, V, stats, mode, exact), V, stats, mode)
    out["A"] = ur.advantage(b.ret, V, stats, b.m)
    return out


@pytest.mark.parametrize("fam,head,n_in,rows", CELLS)
def test_instantiation_at_row_count(fam, head, n_in, rows):
    M = _rows(rows, _waves(fam, head, n_in))
    tag = f"{fam}-{head}{n_in}-M{M}"
    b = _make(head, n_in, M, seed=1000 * n_in + len(rows) + M % 97, xs=3.0 if head == "c" else 2.0)
    bad = []
    _run_cell(bad, tag, fam, b)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- the pair kernel
@pytest.mark.parametrize("rows", SMALL + LARGE)
def test_pair_launch_bit_identical_to_two_passes(rows):
    """mhppo_mlp_train_pair (the default of every continuous head up to 2 M rows; it overwrites
    `value` in place) against the actor pass e and the critic pass e + 1 as two launches, on random
    data: both gradients, both sums and V after the call, bit for bit.  At M = 33 and 32 W C + 33 the
    pair's own outputs also against the float64 reference."""
    from mhppo import ppo
    M = _rows(rows, 4)
    tag = f"pair-c13-M{M}"
    b = _make("c", 13, M, seed=77 + M % 89, xs=3.0)
    _, sc0, V0 = ppo.k_mlp_train(ppo.KIND_CRITIC, b.critic, b.obs, b.ret, m_global=b.m)
    stats = ur.adv_sums(b.ret, V0)
    V0 = V0.clone()
    with torch.no_grad():  # the critic's Adam step e (any update of its weights)
        gen = torch.Generator(device=DEV).manual_seed(M)
        for prm in b.critic.parameters():
            prm.add_(torch.randn(prm.shape, generator=gen, device=DEV) * 1e-3)
    ga, sa = _actor_pass(b, V0, stats, "cont", False)
    gc, sc, V1 = ppo.k_mlp_train(ppo.KIND_CRITIC, b.critic, b.obs, b.ret, m_global=b.m)
    gc, sc, V1 = gc.clone(), sc.clone(), V1.clone()
    b.actor.grad_flat().fill_(7.0)
    b.critic.grad_flat().fill_(7.0)
    V = V0.clone()
    sa2 = torch.zeros(3, dtype=torch.float64, device=DEV)
    sc2 = torch.zeros(3, dtype=torch.float64, device=DEV)
    ga2, gc2, V = ppo.k_mlp_train_pair(b.actor, b.critic, b.obs, b.ret, V, b.act, b.lpo, stats, b.m, sa2, sc2)
    assert torch.equal(ga2, ga), "actor gradient"
    assert torch.equal(gc2, gc), "critic gradient"
    assert torch.equal(V, V1), "V after the call"
    assert torch.equal(sa2, sa) and torch.equal(sc2, sc), "sums"
    if rows in ("33", "grid+33"):
        bad = []
        _check_actor(bad, tag, "pair", b, (ga2.clone(), sa2), V0, stats, "cont")
        _check_critic(bad, tag, "pair", b, (gc2.clone(), sc2, V))
        assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- M = 0
EMPTY = [("critic13", False), ("critic13", True), ("cont", False), ("cont", True), ("critic_d", False),
         ("critic_d", True), ("critic_wide", False), ("counts", False), ("counts", True), ("per_row", False),
         ("per_row", True), ("counts_wide", False), ("pair", False)]


@pytest.mark.parametrize("what,exact", EMPTY, ids=[f"{w}-{'f32' if e else 'default'}" for w, e in EMPTY])
def test_empty_batch_gives_zero_gradient_and_leaves_sums(what, exact):
    """M = 0 (an empty data-parallel shard): the gradient is all zeros and `sums` is untouched, for
    every kind, on either kernel family, and for the pair."""
    from mhppo import ppo
    from mhppo.models import Model_PPO
    torch.manual_seed(0)
    dc = 60 if what.endswith("_wide") else 27
    cont = what in ("critic13", "cont", "pair")
    n_in = 13 if cont else dc
    actor = (Model_PPO(13, 1, 1, mean=-1.0, std=3.0) if cont else Model_PPO(dc, 2, 2)).to(DEV)
    critic = Model_PPO(n_in, 1, 0).to(DEV)
    e = torch.empty(0, device=DEV)
    obs = torch.empty(0, n_in, device=DEV)
    mark = torch.tensor([1.5, -2.5, 3.5], dtype=torch.float64, device=DEV)
    sums, sums2 = mark.clone(), mark.clone()
    stats = torch.tensor([3.0, 11.0], dtype=torch.float64, device=DEV)
    counts = torch.tensor([5.0, 3.0], dtype=torch.float64, device=DEV)
    for net in (actor, critic):
        net.grad_flat().fill_(7.0)
    if what.startswith("critic"):
        g, _, V = ppo.k_mlp_train(ppo.KIND_CRITIC, critic, obs, e, m_global=8.0, exact=exact, sums=sums)
        grads = [(g, critic)]
        assert V.numel() == 0
    elif what == "cont":
        g, _, _ = ppo.k_mlp_train(ppo.KIND_CONT, actor, obs, e, e, e, e, stats, m_global=8.0, exact=exact, sums=sums)
        grads = [(g, actor)]
    elif what == "pair":
        ga, gc, _ = ppo.k_mlp_train_pair(actor, critic, obs, e, e.clone(), e, e, stats, 8.0, sums, sums2)
        grads = [(ga, actor), (gc, critic)]
    else:
        per_row = what == "per_row"
        g, _, _ = ppo.k_mlp_train(ppo.KIND_CHOICE, actor, obs, e, e, e if per_row else None, e, stats,
                                  None if per_row else counts, m_global=8.0, exact=exact, sums=sums)
        grads = [(g, actor)]
    torch.cuda.synchronize()
    for g, net in grads:
        assert g.numel() == net.flat().numel() == ppo.n_params(net.n_in, net.n_out)
        assert torch.count_nonzero(g) == 0
    assert torch.equal(sums, mark) and torch.equal(sums2, mark)


# ---------------------------------------------------------------- trained-policy regimes
# Layer 4 (weights and bias) of a default-init choice actor (torch.manual_seed(net_seed), fixed per
# dc: the spread of the logit gap varies a lot between initialisations) times a per-dc factor, inputs
# 2 randn: the float64 logit gap |y0 - y1| then spreads over both sides of the clamp of the
# probabilities to [eps, 1 - eps] (gap 15.94).  Rows with a gap in [12, 20] are dropped: the band
# straddles the clamp and the float32 rounding of 1 - p to 1.  Below 12 a row is inside the clamp;
# above 20 it is clamped in float64 and in float32 alike, and its gradient is exactly zero.
# dc: (factor, net_seed); on the CPU each leaves 25 % to 55 % of the kept rows in either regime.
SAT_CHOICE = {12: (300.0, 5), 30: (150.0, 1), 54: (150.0, 1), 64: (150.0, 0)}
SAT_CELLS = [pytest.param(f, dc, M, id=f"{f}-d{dc}-M{M}")
             for dc in SAT_CHOICE for f in (("x3", "f32") if dc <= 54 else ("auto", "f32")) for M in (33, 4097)]


@pytest.mark.parametrize("fam,dc,M", SAT_CELLS)
def test_saturated_choice_head(fam, dc, M):
    """A choice actor as a trained policy leaves it: part of the rows inside the clamp of the
    probabilities, part clamped (the `pass` mask zeroes them).  Both regimes hold at least 10 % of
    the rows (asserted on the float64 forward); both modes; the same per-tensor bound."""
    from mhppo import ppo
    scale4, net_seed = SAT_CHOICE[dc]
    tag = f"sat-{fam}-d{dc}-M{M}"
    b = _make("d", dc, M, seed=31 * dc + M, xs=2.0, scale4=scale4, band=(12.0, 20.0), net_seed=net_seed)
    inside, clamped = float((b.gap < 12).double().mean()), float((b.gap > 20).double().mean())
    print(f"UPDM regime {tag} inside={inside:.3f} clamped={clamped:.3f}")
    assert int((b.gap < 12).sum()) + int((b.gap > 20).sum()) == M
    assert inside >= 0.10 and clamped >= 0.10, (inside, clamped)
    bad = []
    _run_cell(bad, tag, fam, b)
    assert not bad, "\n".join(bad)
    # the clamped rows on their own: an exactly zero gradient in either mode
    sel = b.gap > 20
    c = _Batch()
    c.actor, c.critic, c.head, c.n_in = b.actor, b.critic, "d", dc
    c.obs, c.ret, c.act, c.lpo = (t[sel].contiguous() for t in (b.obs, b.ret, b.act, b.lpo))
    c.M = int(sel.sum())
    c.m = float(c.M)
    assert c.M >= 3
    exact = fam == "f32"
    _, _, V = ppo.k_mlp_train(ppo.KIND_CRITIC, c.critic, c.obs, c.ret, m_global=c.m, exact=exact)
    stats = ur.adv_sums(c.ret, V)
    for mode in ("counts", "per_row"):
        c.actor.grad_flat().fill_(7.0)
        ga, _ = _actor_pass(c, V, stats, mode, exact)
        assert torch.count_nonzero(ga) == 0, f"{tag} {mode}: clamped rows alone give a non-zero gradient"
        r64, _ = _actor_refs(c, V, stats, mode)
        assert all(torch.count_nonzero(g) == 0 for g in r64["grads"])


@pytest.mark.parametrize("fam", ["x3", "f32"])
@pytest.mark.parametrize("M", [33, 4097])
def test_saturated_continuous_actor(fam, M):
    """Layer 4 of the continuous actor (torch.manual_seed(9)) times 30, inputs 3 randn: part of the rows with |y| < 2 (tanh
    unsaturated), part with tanhf(y) == +-1 in float32 (|y| > 9.5: 1 - t * t is exactly 0 there).
    Rows with |y| in [7, 9.5] are dropped; at least 10 % of the rows in each regime."""
    tag = f"sat-{fam}-c13-M{M}"
    b = _make("c", 13, M, seed=5 + M, xs=3.0, scale4=30.0, band=(7.0, 9.5), net_seed=9)
    live, flat = float((b.gap < 2).double().mean()), float((b.gap > 9.5).double().mean())
    print(f"UPDM regime {tag} unsaturated={live:.3f} saturated={flat:.3f}")
    assert live >= 0.10 and flat >= 0.10, (live, flat)
    assert bool((torch.tanh(b.gap[b.gap > 9.5].float()) == 1.0).all())
    bad = []
    _run_cell(bad, tag, fam, b)
    assert not bad, "\n".join(bad)


# logp_old = float32(logp64 - d): none of these d is within 0.03 of ln 0.8 = -0.2231 or ln 1.2 =
# 0.1823, so the float32 rounding of logp cannot move a row across a clip bound
DELTAS = (-0.5, -0.35, -0.1, 0.0, 0.1, 0.3, 0.5)
CLIP_CELLS = [pytest.param(f, h, n, M, id=f"{f}-{h}{n}-M{M}")
              for (f, h, n) in (("x3", "c", 13), ("f32", "c", 13), ("x3", "d", 27), ("f32", "d", 27), ("auto", "d", 60))
              for M in (257, 4097)]


@pytest.mark.parametrize("fam,head,n_in,M", CLIP_CELLS)
def test_both_sides_of_the_clip(fam, head, n_in, M):
    """Ratios below, inside and above [0.8, 1.2] for both signs of the advantage: at least 5 % of the
    rows in each of the six cells, counted on the reference's ratio (the row's own action's for the
    choice head) and its normalised A."""
    tag = f"clip-{fam}-{head}{n_in}-M{M}"
    b = _make(head, n_in, M, seed=900 + n_in + M, xs=3.0 if head == "c" else 2.0, deltas=DELTAS)
    bad = []
    out = _run_cell(bad, tag, fam, b)
    A = out["A"]
    d = out["cont"]["d"] if head == "c" else out["per_row"]["d"].gather(1, b.act.long()[:, None])[:, 0]
    side = torch.where(d < ur.LN_LO, 0, torch.where(d > ur.LN_HI, 2, 1))
    assert float((d - ur.LN_LO).abs().min()) > 0.03 and float((d - ur.LN_HI).abs().min()) > 0.03
    for s in range(3):
        for sign in (-1, 1):
            frac = float(((side == s) & (torch.sign(A) == sign)).double().mean())
            print(f"UPDM regime {tag} side={s} sign={sign:+d} frac={frac:.3f}")
            assert frac >= 0.05, (s, sign, frac)
    assert not bad, "\n".join(bad)
