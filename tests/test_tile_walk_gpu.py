"""The forward-only MFMA kernels past one tile per wave: k_mlp_forward<1|2> and k_ppo_diag<1|2>
(csrc/mlp_infer.hip) and k_policy_decide / _act / _sample_decide / _sample_act (csrc/policy_infer.hip) at
row counts where a wave walks several 32-row tiles grid-stride (a launch is capped at 512 blocks of 4
waves = 2 048 wave slots), which tests/test_infer_gpu.py (M <= 4 099: one step per wave) and
tests/test_policy_gpu.py / test_policy_sample_gpu.py (2 050 tiles: two waves take a second one) never do.

References cost nothing: every output is a function of its own row (the Philox launches: and of the
row's flat index), so the host build runs on a small pool (the 4 099 rows of test_infer_gpu's references,
the 4 480 harvested observation rows of test_policy_gpu.harvest) and the M device rows are pool[idx],
idx = default_rng(seed).integers(0, len(pool), M), every per-row input gathered by the same idx; expected is
ref_pool[idx], for the diagnostics terms_pool[idx].sum(0) in float64.  Such an idx hits every pool row and
rows 65 536 apart almost never coincide (asserted), so a tile read from or written to another step shows.
Only the Philox forms run the host build on all M rows (tools/hostpolicy.cpp threads its row loops).

mlp_forward / ppo_diag (the block-synchronous walk, 65 536 rows per step): M = 65 536 (the grid exactly at
its cap, one step), 65 537 (step 2 exists for block 0 alone: one live wave with a 1-row tile, three dead
waves at the loop's barriers) and 131 239 = 2 x 65 536 + 5 x 32 + 7 (a third step with one full block, one
half-live block and a 7-row last tile; acc[] carried over three steps; k_diag_fold over the capped 512
partials, two per thread).  The policy launches (wave-independent walk): M with (B + 1) x 2 048 + 5 act
tiles, B = 64 / G the tiles one Philox draw serves and G = 32 / P the (row, slot) groups of a tile, the last
tile ragged: every wave takes B + 1 or B + 2 tiles, redraws its normals once, and the last redraw reaches
past the launch's units; G = 32, 16 and 10 (P = 3: four lanes draw nothing); the decide kernels take 3 to 7
tiles per wave at the same M.

Out of reach: tile_div's 64-bit branch (more than INT32_MAX triples or groups in one launch) needs more
than 2^31 triples.

Mutants (scratch builds of the library, never committed; each changes only which in-bounds value is read
or whether a term is added), the kernel's older tests and this module run once against each on an MI355X:
  (a) k_mlp_forward stages, in steps after the first, the rows of its first-step tile (stores left alone):
      tests/test_infer_gpu.py 0 of 92 fail; here 8 of 25: test_forward_walk_bit_identical_to_host at 65 537
      and 131 239 for all four nets (65 536, one step, passes).
  (b) k_ppo_diag accumulates a row's terms only in a block's first step: tests/test_infer_gpu.py 0 of 92
      fail; here 4 of 25: all of test_diag_walk_sums_vs_host (the determinism test rightly passes: the
      mutant is deterministic).
  (c) k_policy_sample_act draws its normals only at a wave's first tile: tests/test_policy_sample_gpu.py
      0 of 17 fail; here 3 of 25: test_policy_walk_philox for G = 32, 16 and 10.

Wall time of each test on an MI355X (pytest --durations, call phase; the module's 25 tests: 4.2 s in all):
test_forward_walk_bit_identical_to_host 0.01 - 0.03 s a case (0.38 s the first: the device's start-up),
test_diag_walk_sums_vs_host 0.01 - 0.16 s (the larger: the pool's reference), test_diag_walk_deterministic_
and_streams 0.01 - 0.09 s, test_policy_walk_pool_gathered 0.15 / 0.32 / 0.21 s and test_policy_walk_philox
0.17 / 0.32 / 0.33 s for 4cars 4/1/2, scalable 8/2/4 and scalable 4/3/2, test_row_counts_reach_the_walk 0.01 s.
"""
import os
import sys

import numpy as np
import pytest
import torch

import infer_common as ic
import test_infer_gpu as tig
import test_policy_gpu as tpg
import test_policy_sample_gpu as tps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu

STEP_ROWS = 512 * 4 * 32  # rows of one step of the capped grid: 65 536
NET_MS = (STEP_ROWS, STEP_ROWS + 1, 2 * STEP_ROWS + 5 * 32 + 7)
FWD_CASES = [(1, 13), (0, 64), (2, 54), (2, 5)]
DIAG_POOLS = [(1, 13, 0.05, 9112), (2, 54, 0.1, 6201)]  # (akind, n_in, sigma, pool seed): 4 099 rows each
POOL_M = max(tig.MS)
IDX_SEED = 2718
WAVE_SLOTS = 512 * 4
# (shape, M): (B + 1) 2048 + 5 act tiles, the last one ragged
POLICY_CASES = [(("4cars", 4, 1, 2), 49191), (("scalable", 8, 2, 4), 20489), (("scalable", 4, 3, 2), 35852)]
POLICY_IDS = ["%s_%d%d%d" % s for s, _ in POLICY_CASES]

_IDX, _DIAG, _POL = {}, {}, {}


def gather_idx(n_pool, M):
    """The pool row of each of the M device rows."""
    if (n_pool, M) not in _IDX:
        idx = np.random.default_rng(IDX_SEED).integers(0, n_pool, M)
        assert np.unique(idx).size > 0.98 * n_pool  # (nearly) the whole pool is among the device rows
        if M > STEP_ROWS + 32:  # a row and the one a step later differ almost always
            assert (idx[STEP_ROWS:] == idx[:-STEP_ROWS]).mean() < 1e-3
        _IDX[(n_pool, M)] = idx
    return _IDX[(n_pool, M)]


# ------------------------------------------------------------------ 1. mlp_forward
def test_row_counts_reach_the_walk():
    """The arithmetic the cases rest on: steps per block of the net kernels, tiles per wave of the policy's."""
    tiles = [(M + 31) // 32 for M in NET_MS]
    assert tiles == [WAVE_SLOTS, WAVE_SLOTS + 1, 2 * WAVE_SLOTS + 6] and [M % 32 for M in NET_MS] == [0, 1, 7]
    assert np.unique(gather_idx(POOL_M, NET_MS[2])).size == POOL_M  # every pool row is among the device rows
    import hostpolicy as hp
    for (shape, M), G in zip(POLICY_CASES, (32, 16, 10)):
        od, S, P, dc = hp.dims(hp.cfg(*shape))
        assert G == 32 // P
        B, U, Q = 64 // G, M * S, M * S * P
        act_tiles, dec_tiles = (U + G - 1) // G, (Q + 31) // 32
        assert act_tiles == (B + 1) * WAVE_SLOTS + 5 and U % G != 0 and Q % 32 != 0
        assert 3 * WAVE_SLOTS < dec_tiles < 7 * WAVE_SLOTS
        # a wave's redraw (at its tile B, B strides on) draws for its tiles B .. 2 B - 1: the first waves own
        # tile B + 1 (they take B + 2 tiles), the last wave's lies past the end (the draw's `tu < U`)
        assert (B + 1) * WAVE_SLOTS < act_tiles <= (B + 1) * WAVE_SLOTS + WAVE_SLOTS - 1 and B >= 2


@pytest.mark.parametrize("M", NET_MS)
@pytest.mark.parametrize("kind,n_in", FWD_CASES)
def test_forward_walk_bit_identical_to_host(kind, n_in, M):
    W, X, ref = tig._fwd_ref(kind, n_in)
    idx = gather_idx(len(X), M)
    net = tig.gpu_net(kind, n_in, W)
    out = net.forward_rows(tig.t(X[idx]))
    assert out.shape == ((M, 2) if kind == 2 else (M,)) and out.dtype == torch.float32
    assert torch.equal(out.cpu(), torch.from_numpy(ref[idx]))


# ------------------------------------------------------------------ 2. ppo_diag
def _diag_pool(akind, n_in, sigma, seed):
    key = (akind, n_in, sigma, seed)
    if key not in _DIAG:
        c = ic.diag_case(akind, n_in, POOL_M, sigma, seed)
        _DIAG[key] = (c, ic.host_terms(c))
    return _DIAG[key]


def _gathered(c, idx):
    return dict(c, M=len(idx), **{k: np.ascontiguousarray(c[k][idx]) for k in ("X", "act", "logp_old", "ret")})


@pytest.mark.parametrize("M", NET_MS[1:])
@pytest.mark.parametrize("akind,n_in,sigma,seed", DIAG_POOLS)
def test_diag_walk_sums_vs_host(akind, n_in, sigma, seed, M):
    """test_infer_gpu.test_diag_sums_vs_host's assertions and bars.  Reordering M <= 131 239 doubles costs at
    most M 2^-53 = 1.5e-11 of sum |term|: the 1e-10 bar holds at this M."""
    from mhppo import ppo
    c, (d, terms, lp) = _diag_pool(akind, n_in, sigma, seed)
    idx = gather_idx(POOL_M, M)
    d, terms, lp = d[idx], terms[idx], lp[idx]
    # the reference alone: a real mix of clipped rows, none at a boundary
    frac = terms[:, 2].mean()
    near = min(np.abs(d - ic.LN_0_8).min(), np.abs(d - ic.LN_1_2).min())
    print(f"reference clip fraction {frac:.3f}, nearest row to a boundary {near:.3g}")
    assert 0.05 <= frac <= 0.95
    assert near > 1e-6
    got = ppo.k_ppo_diag(tig.make_head(_gathered(c, idx))).cpu().numpy()
    want, scale = terms.sum(0), np.abs(terms).sum(0)
    slack = 2.0 ** -22 * np.abs(lp.astype(np.float64)).sum() if akind == 2 else 0.0  # logf: <= 1 ulp each side
    for k in range(10):
        print(f"term {k}: gpu {got[k]!r} host {want[k]!r} sum |term| {scale[k]:.3g}")
    assert got[ppo.DIAG_CLIP] == want[ppo.DIAG_CLIP]
    for k in (ppo.DIAG_DSUM, ppo.DIAG_K3, ppo.DIAG_RATIO):
        assert abs(got[k] - want[k]) <= slack + 1e-10 * scale[k], k
    for k in (ppo.DIAG_ENT, ppo.DIAG_E, ppo.DIAG_E2, ppo.DIAG_G, ppo.DIAG_G2, ppo.DIAG_V):
        assert abs(got[k] - want[k]) <= 1e-10 * scale[k], k
    if akind == 1:
        assert got[ppo.DIAG_ENT] == 0.0


@pytest.mark.parametrize("akind,n_in,sigma,seed", DIAG_POOLS)
def test_diag_walk_deterministic_and_streams(akind, n_in, sigma, seed):
    from mhppo import _lib, ppo
    M = NET_MS[2]
    assert _lib.lib().mhppo_ppo_diag_work_bytes(M) == ppo.DIAG_N * 512 * 8  # the fold's 512 partials per term
    c, _ = _diag_pool(akind, n_in, sigma, seed)
    h = tig.make_head(_gathered(c, gather_idx(POOL_M, M)))
    s1 = ppo.k_ppo_diag(h)
    s2 = ppo.k_ppo_diag(h)
    assert torch.equal(s1, s2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s3 = ppo.k_ppo_diag(h)
    side.synchronize()
    assert torch.equal(s1, s3)


# ------------------------------------------------------------------ 3. the policy launches
def _policy(shape, M):
    """Per shape, once: the config, the two policies (continuous nets of mean -1 and of mean 1, whose
    candidates lie on both sides of 2.0), the harvested pool, the gathered device rows and pool-level noise."""
    if shape not in _POL:
        import hostpolicy as hp
        from mhppo.models import Model_PPO
        from mhppo.policy import Policy
        c = hp.cfg(*shape)
        od, S, P, dc = hp.dims(c)
        ac, aw, ad = tpg.nets(dc)
        torch.manual_seed(6)
        hi = (Model_PPO(13, 1, 1, mean=1.0, std=3.0).cuda(), Model_PPO(13, 1, 1, mean=1.0, std=3.0).cuda())
        pool = tpg.harvest(*shape).cpu().numpy()
        n = len(pool)
        idx = gather_idx(n, M)
        rng = np.random.default_rng(5)
        s = dict(c=c, od=od, S=S, P=P, dc=dc, M=M, idx=idx, pool=pool, o_g=np.ascontiguousarray(pool[idx]),
                 lo=Policy(*shape, ac, aw, ad), hi=Policy(*shape, hi[0], hi[1], ad),
                 wd=ad.packed().cpu().numpy(), w_lo=[x.packed().cpu().numpy() for x in (ac, aw)],
                 w_hi=[x.packed().cpu().numpy() for x in hi],
                 u=rng.uniform(size=(n, S, P)).astype(np.float32), eps=rng.normal(size=(n, S)).astype(np.float32),
                 forced=rng.integers(0, 2, (n, S, P)).astype(np.int32))
        s["obs"] = tig.t(s["o_g"])
        _POL[shape] = s
    assert _POL[shape]["M"] == M
    return _POL[shape]


def _rows(ref, idx, keys):
    return {k: ref[k][idx] for k in keys}


@pytest.mark.parametrize("shape,M", POLICY_CASES, ids=POLICY_IDS)
def test_policy_walk_pool_gathered(shape, M):
    """The deterministic launches and the tape / forced forms: the host rule on the pool, gathered."""
    import hostpolicy as hp
    s = _policy(shape, M)
    c, idx, pool, obs, pol, wd = s["c"], s["idx"], s["pool"], s["obs"], s["lo"], s["wd"]
    # decide, act on the decided and on a mixed a_d
    ref_a, ref_p = hp.decide(c, wd, pool, probs=True)
    assert 0 < ref_a[idx].sum() < ref_a[idx].size
    a, p = tpg.raw_decide(pol, obs, M)
    assert tpg.same_bits(a, ref_a[idx]), "a_d"
    assert tpg.same_bits(p, ref_p[idx]), "probs"
    for name, v in (("decided", ref_a), ("mixed", s["forced"])):
        ref = hp.act(c, *s["w_lo"], pool, v)
        out = tpg.raw_act(pol, obs, tig.t(v[idx]), M)
        assert tpg.same_bits(out, ref[idx]), name
    # sample_decide on a gathered u tape and on gathered forced decisions, every optional output on
    ref_u = hp.sample_decide(c, wd, pool, u=s["u"])
    ref_f = hp.sample_decide(c, wd, pool, forced=s["forced"])
    assert ref_u["status"] == 0 and ref_f["status"] == 0
    assert 0 < ref_u["a_d"][idx].sum() < ref_u["a_d"][idx].size
    tape = tig.t(s["u"][idx])
    tps.check_decide(tps.raw_decide(pol, obs, M, tps.noise_struct(tape=tape)), _rows(ref_u, idx, tps.DEC_KEYS), M, "u")
    forced = tig.t(s["forced"][idx])
    tps.check_decide(tps.raw_decide(pol, obs, M, tps.noise_struct(forced=forced)), _rows(ref_f, idx, tps.DEC_KEYS), M,
                     "forced")
    # sample_act on a gathered eps tape, feat_c on
    ref = hp.sample_act(c, *s["w_lo"], pool, ref_u["a_d"], ref_u["closest"], eps=s["eps"])
    assert ref["status"] == 0
    eps = tig.t(s["eps"][idx])
    got = tps.raw_act(pol, obs, tig.t(ref_u["a_d"][idx]), tig.t(ref_u["closest"][idx]), M, tps.noise_struct(tape=eps))
    assert set(got) == set(tps.ACT_KEYS)
    for name in got:
        assert tpg.same_bits(got[name], ref[name][idx]), name


@pytest.mark.parametrize("shape,M", POLICY_CASES, ids=POLICY_IDS)
def test_policy_walk_philox(shape, M):
    """The in-kernel Philox forms: the noise is a function of the flat index, so the host build sees all M rows.
    sample_act runs the mean-1 nets on a mixed a_d (the existing test's (1.0, "mixed", "philox") run)."""
    import hostpolicy as hp
    from mhppo.policy import noise_key
    s = _policy(shape, M)
    c, idx, o_g, obs, S, P, od = s["c"], s["idx"], s["o_g"], s["obs"], s["S"], s["P"], s["od"]
    key = noise_key(tps.SEED, tps.ITER)
    mixed = np.ascontiguousarray(s["forced"][idx])
    ref_dec = hp.sample_decide(c, s["wd"], o_g, key=key, first_env=tps.FIRST)
    closest = ref_dec["closest"]
    eps_dev = tps.device_normals(key, tps.FIRST, tps.STEP, M, S)
    ref_act = hp.sample_act(c, *s["w_hi"], o_g, mixed, closest, eps=eps_dev.cpu().numpy(), mean=1.0)
    assert ref_dec["status"] == 0 and ref_act["status"] == 0

    # what the compared rows must contain (conditions of the test, judged on the host build alone)
    assert 0 < ref_dec["a_d"].sum() < ref_dec["a_d"].size
    ped_there = np.ones((M, P), bool)
    if shape[0] == "scalable":
        ped_there = o_g[:, od - 9 * P:].reshape(M, P, 9)[:, :, 7] != 0
        assert (~ped_there).any(), "no absent pedestrian among the rows"
        assert (ref_dec["exist"] == 0).any(), "no absent car among the rows"
    # a = loc + L * 0: the fold's loc itself (per row: computed on the pool, gathered)
    pool_closest = hp.sample_decide(c, s["wd"], s["pool"], forced=s["forced"])["closest"]
    assert tpg.same_bits(pool_closest[idx], closest)
    loc_hi = hp.sample_act(c, *s["w_hi"], s["pool"], s["forced"], pool_closest, eps=np.zeros_like(s["eps"]),
                           mean=1.0)["act"][idx]
    assert ((loc_hi == 2.0) & ped_there.any(1)[:, None]).any(), "no slot whose every candidate exceeds 2.0"
    assert (loc_hi < 2.0).any()
    if P > 1:
        assert (ref_act["feat_c"] != hp.features(c, o_g)[:, :, 0]).any(), "no slot with sel > 0"

    tps.check_decide(tps.raw_decide(s["lo"], obs, M, tps.noise_struct(key=key, first_env=tps.FIRST)), ref_dec, M,
                     "philox")
    d_mixed, d_closest = tig.t(mixed), tig.t(closest)
    got = tps.raw_act(s["hi"], obs, d_mixed, d_closest, M, tps.noise_struct(key=key, first_env=tps.FIRST, t=tps.STEP))
    tape = tps.raw_act(s["hi"], obs, d_mixed, d_closest, M, tps.noise_struct(tape=eps_dev))
    assert set(got) == set(tps.ACT_KEYS)
    for name in got:
        assert tpg.same_bits(got[name], ref_act[name]), (name, "host build on the library's normals")
        assert tpg.same_bits(got[name], tape[name]), (name, "the device's tape launch on the same normals")
