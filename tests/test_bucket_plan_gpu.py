"""mhppo_bucket_plan + mhppo_bucket_scatter_sums (bucket_segments' native GPU path) against the
torch path (bucket_segments_torch) on the same synthetic CUDA batches: positions, sizes, counts and
the choice actions equal, every float row bitwise equal, the float64 reward sums within 1e-12
relative (a different but fixed summation order).  Shapes: the smallest that reach each branch —
one block and several, NS ragged against and straddling the plan's 256-segment blocks, the
scatter's 64-segment blocks and the one-block scan's 256-block tiles, several pedestrians with and
without fix_bucket, the compact record layout, empty buckets, and every cross count mod 4 (the wait
bucket's 4-segment aligned start)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NF_C = 13


def make_batch(N, S, P, T, dc=5, seed=0, p_exist=0.8, compact=False, n_cross=None, a_fill=None):
    """A RolloutBatch of random records (no env).  compact: about 40 % of the car slots absent, the
    present ones' records contiguous (rec_of).  n_cross (P == 1): every segment exists and exactly
    the first n_cross are cross.  a_fill: every choice action = a_fill."""
    from mhppo.rollout import RolloutBatch
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + S + P + T)
    NS = N * S
    a_d = torch.randint(0, 2, (N, S, P), generator=g, dtype=torch.int32)
    exist = (torch.rand(N, S, generator=g) < p_exist)
    if a_fill is not None:
        a_d.fill_(a_fill)
    if n_cross is not None:
        assert P == 1
        a_d = (torch.arange(NS) >= n_cross).to(torch.int32).reshape(N, S, 1)
        exist.fill_(True)
    rec_of = None
    if compact:
        present = torch.rand(NS, generator=g) < 0.6
        exist &= present.reshape(N, S)
        rec_of = torch.where(present, torch.cumsum(present, 0) - 1, -1).to(torch.int32).cuda()
    kw = dict(
        a_d=a_d, closest=torch.randint(0, P, (N, S), generator=g, dtype=torch.int32), exist=exist.to(torch.uint8),
        ep_min=-torch.rand(N, S, generator=g, dtype=torch.float64) - 0.1,
        feat_d=torch.randn(N, S, P, dc, generator=g), logp_d=torch.randn(N, S, P, generator=g),
        probs_d=torch.zeros(N, S, P, 2), obs_c_tm=torch.randn(T, N, S, NF_C, generator=g),
        act_tm=torch.randn(T, N, S, generator=g), logp_tm=torch.randn(T, N, S, generator=g),
        # rewards of one sign (as the env's are): the sums' relative bound then tests the
        # summation, not a cancellation
        rew_tm=-torch.rand(T, N, S, generator=g, dtype=torch.float64) - 0.05)
    return RolloutBatch(**{k: v.cuda() for k, v in kw.items()}, rec_of=rec_of, N=N, S=S, P=P, T=T)


def bits(x):
    return x.contiguous().view({4: torch.int32, 8: torch.int64, 1: torch.int8}[x.element_size()])


def reward_sums(c, w, d):
    """Algo_PPO.train's torch reductions."""
    return torch.stack([c["rew"].float().double().sum(), w["rew"].float().double().sum(), d["ret"].double().sum()])


def check(batch, fix_bucket=False):
    from mhppo.rollout import bucket_plan, bucket_segments_native, bucket_segments_torch
    NS = batch.N * batch.S
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    ref_plan = {}
    ref = bucket_segments_torch(batch, fix_bucket, status, plan_out=ref_plan)
    out = bucket_segments_native(batch, fix_bucket, status)
    # the plan's integers
    plan = bucket_plan(batch, fix_bucket, status)
    torch.cuda.synchronize()
    assert plan["pos"].dtype == torch.int64 and plan["bucket"].dtype == torch.int8
    assert torch.equal(plan["pos"], ref_plan["pos"])
    wait = ref_plan["wait"]
    if batch.rec_of is not None:  # per record
        idx = torch.where(batch.rec_of >= 0, batch.rec_of, NS).long()
        wait = torch.zeros(NS + 1, dtype=torch.bool, device="cuda").scatter_(0, idx, wait)[:NS]
    assert torch.equal(plan["bucket"], wait.to(torch.int8))
    assert plan["info"][:4].tolist() == [ref[0]["n_seg"], ref[1]["n_seg"], ref[2]["n_seg"], 0]
    # the batches
    for name, a, b in (("cross", out[0], ref[0]), ("wait", out[1], ref[1])):
        assert a["n_seg"] == b["n_seg"], name
        for k in ("obs", "act", "logp", "ret", "rew"):
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (name, k)
            assert torch.equal(bits(a[k]), bits(b[k])), (name, k)
    a, b = out[2], ref[2]
    assert a["n_seg"] == b["n_seg"]
    for k in ("obs", "act", "logp", "ret"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert a["counts"].dtype == torch.float64 and torch.equal(a["counts"], b["counts"])
    want, got = reward_sums(*ref), a["rew_sums"]
    print("reward sums", got.tolist(), "torch", want.tolist())
    assert bool(((got - want).abs() <= 1e-12 * want.abs()).all())
    return out


@pytest.mark.parametrize("N,S,P,T", [(1, 4, 1, 5), (3, 4, 1, 5), (257, 4, 1, 80), (5, 3, 2, 17)])
def test_plan_matches_torch_small_and_ragged(N, S, P, T):
    check(make_batch(N, S, P, T))


# NS = N at S = 1: the scatter's 64-segment blocks, the plan's 256-segment blocks (one and two of
# them), and the scan's tiles of 256 blocks (NS = 65536: one tile exactly, +1: a second tile)
@pytest.mark.parametrize("NS", [63, 64, 65, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537])
def test_plan_block_boundaries(NS):
    check(make_batch(NS, 1, 1, 2, dc=3))


@pytest.mark.parametrize("fix_bucket", [False, True])
def test_plan_three_pedestrians(fix_bucket):
    check(make_batch(70, 4, 3, 5, dc=7), fix_bucket)


@pytest.mark.parametrize("fix_bucket", [False, True])
def test_plan_compact_layout(fix_bucket):
    check(make_batch(90, 8, 2, 18, dc=54, compact=True), fix_bucket)


@pytest.mark.parametrize("case", ["all_cross", "all_wait", "none_exist"])
def test_plan_empty_buckets(case):
    kw = dict(all_cross=dict(a_fill=0, p_exist=2.0), all_wait=dict(a_fill=1, p_exist=2.0),
              none_exist=dict(p_exist=-1.0))[case]
    c, w, d = check(make_batch(67, 4, 1, 5, **kw))
    assert (c["n_seg"], w["n_seg"], d["n_seg"]) == dict(all_cross=(268, 0, 268), all_wait=(0, 268, 268),
                                                        none_exist=(0, 0, 0))[case]


@pytest.mark.parametrize("n_cross", [4, 5, 6, 7])
def test_plan_wait_bucket_start(n_cross):
    """w0 = the cross count rounded up to a multiple of 4."""
    from mhppo.rollout import bucket_plan
    batch = make_batch(3, 4, 1, 5, n_cross=n_cross)
    c, w, _ = check(batch)
    assert (c["n_seg"], w["n_seg"]) == (n_cross, 12 - n_cross)
    pos = bucket_plan(batch)["pos"].tolist()
    w0 = (n_cross + 3) // 4 * 4
    assert pos == list(range(n_cross)) + list(range(w0, w0 + 12 - n_cross))


def test_plan_second_call_identical_bytes():
    from mhppo.rollout import bucket_segments_native
    batch = make_batch(300, 4, 2, 33)
    a = bucket_segments_native(batch)
    b = bucket_segments_native(batch)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            if torch.is_tensor(x[k]):
                assert torch.equal(bits(x[k]), bits(y[k])), k
            else:
                assert x[k] == y[k], k


def test_plan_returns_status_word():
    """The rollout's NaN-flag word comes back with the sizes: raised on and cleared."""
    from mhppo import _lib
    from mhppo.rollout import bucket_segments
    batch = make_batch(3, 4, 1, 5)
    status = torch.full((1,), 2, dtype=torch.int32, device="cuda")
    with pytest.raises(_lib.MhppoNaNError):
        bucket_segments(batch, status=status)
    assert int(status.item()) == 0
    bucket_segments(batch, status=status)
