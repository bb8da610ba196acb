"""The summation orders of the small kernels, to the bit (csrc/block_prims.h): every float64 sum
below is compared as int64 against the numpy restatement of its order (tests/fold_ref.py), on
inputs normal * exp(normal(0, 3)) whose sums show their order (tests/test_fold_order_host.py), and
the head lists / record ranks against torch at block boundaries.  All through the Python bindings.
Shapes: the smallest that reach one block and several, a ragged tail, the fold's second strided
round and its second / fourth chain."""
import ctypes

import numpy as np
import pytest
import torch

import fold_ref as F

pytestmark = pytest.mark.gpu


def same_bits(got, want, what):
    got = np.ascontiguousarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    print(what, "got", got.tolist(), "want", want.tolist())
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), what


# 1. k_fold<256, 1, add> (and block_reduce_store<2>) through ppo.k_adv_stats
@pytest.mark.parametrize("M", F.ADV_M)
def test_adv_stats_bits(M):
    from mhppo import ppo
    rng = np.random.default_rng(M)
    ret, val = F.heavy(rng, M).astype(np.float32), F.heavy(rng, M).astype(np.float32)
    got = ppo.k_adv_stats(torch.from_numpy(ret).cuda(), torch.from_numpy(val).cuda())
    same_bits(got, F.adv_stats(ret, val), f"adv_stats M={M}")


# 2. k_fold<1024, 4, write> through EvalStats: the 33 N accumulators at the head of the state
@pytest.mark.parametrize("N", F.EVS_N)
def test_eval_stats_fold_bits(N):
    from mhppo.env import VecCrosswalk
    from mhppo.rollout import EvalStats
    from mhppo.stats import EVS_N
    assert EVS_N == 33
    acc = EvalStats(VecCrosswalk("coop", N, 2, 1, 2, seed_base=1))
    acc.begin()
    x = F.heavy(np.random.default_rng(N), (EVS_N, N))
    acc.state[:EVS_N * N].copy_(torch.from_numpy(x).reshape(-1))
    same_bits(acc.fold(), F.fold(x, 1024, 4), f"eval_stats_fold N={N}")


# 3. k_fold<1024, 4, add> and the scatter's partials through mhppo_bucket_scatter_sums; the
# choice sum covers k_plan_count's tree and k_plan_scan's fold
@pytest.mark.parametrize("NS,T", F.SCATTER_NS_T)
def test_bucket_reward_sums_bits(NS, T):
    from mhppo.rollout import bucket_segments_native
    from test_bucket_plan_gpu import make_batch
    batch = make_batch(NS, 1, 1, T, dc=3)
    rng = np.random.default_rng(NS + T)
    rew, ep = F.heavy(rng, (T, NS, 1)), F.heavy(rng, (NS, 1))
    batch.rew_tm = torch.from_numpy(rew).cuda()
    batch.ep_min = torch.from_numpy(ep).cuda()
    got = bucket_segments_native(batch)[2]["rew_sums"]
    torch.cuda.synchronize()
    exist = batch.exist.cpu().numpy().reshape(-1) != 0
    wait = batch.a_d.cpu().numpy().reshape(-1) > 0  # P = 1: the car's own choice
    want = np.concatenate([F.scatter_sums(rew[:, :, 0], exist, wait), [F.plan_ep_sum(ep, exist)]])
    same_bits(got, want, f"rew_sums NS={NS} T={T}")


# 4. head lists and record ranks at block boundaries
def _begin(variant, N, nb_car, nb_ped, nb_lines):
    """mhppo_rollout_begin with a random forced choice -> (rollout, a_d as forced)."""
    from mhppo import _lib
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    from mhppo.rollout import RolloutGPU
    venv = VecCrosswalk(variant, N, nb_car, nb_ped, nb_lines, seed_base=3)
    ro = RolloutGPU(venv, T=2)
    g = torch.Generator().manual_seed(N)
    fa = torch.randint(0, 2, (ro.N, ro.S, ro.P), generator=g, dtype=torch.int32).cuda()
    torch.manual_seed(0)
    mc, keep = Model_PPO(ro.dc, 2, 2).cuda().mlp_desc()
    _lib.check(_lib.lib().mhppo_rollout_begin(venv.handle, ctypes.byref(mc), _lib.ptr(ro.u), _lib.ptr(fa),
                                              ctypes.byref(ro._bufs), _lib.stream_ptr(device=venv.device)))
    torch.cuda.synchronize()
    del keep
    return ro, fa


def _check_rows(ro, fa):
    R = ro.N * ro.S * ro.P
    assert torch.equal(ro.a_d, fa)
    a = fa.reshape(-1)
    cross, wait = torch.nonzero(a == 0).reshape(-1), torch.nonzero(a != 0).reshape(-1)
    rows = ro.rows
    assert rows[R].item() == cross.numel() and rows[R + 1].item() == wait.numel()
    assert torch.equal(rows[:cross.numel()].long(), cross)
    assert torch.equal(rows[cross.numel():R].long(), wait)


# coop 2/1/2 has two rows per env: N = 126, 128, 130 are R = 252, 256, 260 rows (one 256-row block
# ragged, exact, and a second), N = 32770 is 257 blocks (k_head_place's second strided round over
# the block counts); N = 63 .. 16385 stay below those boundaries (one block; 129 blocks)
@pytest.mark.parametrize("N", [63, 64, 65, 16385, 126, 128, 130, 32770])
def test_head_lists_coop(N):
    ro, fa = _begin("coop", N, 2, 1, 2)
    assert ro.N * ro.S * ro.P == 2 * N
    _check_rows(ro, fa)


# scalable 4/2/2 has four segments of two rows per env: N = 31, 32, 33 are R = 248, 256, 264 rows,
# N = 63, 64, 65 are NS = 252, 256, 260 segments (k_flag_rank's block boundary), N = 16449 is 258
# blocks of segments (the last block's second strided round over the 257 counts before it)
@pytest.mark.parametrize("N", [31, 32, 33, 63, 64, 65, 16449])
def test_head_lists_and_record_ranks_scalable(N):
    ro, fa = _begin("scalable", N, 4, 2, 2)
    _check_rows(ro, fa)
    NS = ro.N * ro.S
    assert ro.compact and NS == 4 * N and ro.P == 2
    f = ro.exist.reshape(-1) != 0
    assert 0 < int(f.sum()) < NS
    before = torch.cumsum(f.int(), 0, dtype=torch.int32) - f.int()  # flagged segments before s
    assert torch.equal(ro.rec_buf[:NS], torch.where(f, before, torch.full_like(before, -1)))
    pre = torch.cat([before, f.sum(dtype=torch.int32).reshape(1)])[::ro.S]  # before segment g S, g = 0 .. N
    assert torch.equal(ro.rec_buf[NS:NS + N + 1], pre)
