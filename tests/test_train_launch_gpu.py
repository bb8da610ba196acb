"""The launch layer of the train passes (mhppo/ppo.py) on three small heads built directly with
ppo.Head, no env: a continuous 13 -> 1 head with 70 rows (three tiles, the last ragged), a
continuous 13 -> 1 head with NO local rows of a global batch of 64 (an empty data-parallel shard)
and a choice 20 -> 2 head with 45 rows and global counts.

1. The launch record (ppo.TRAIN_EVENTS, which bench.py computes the train roofline from): the list
   of (kind, n_in, rows) of train_epochs(heads, 2), pairs on and off, and of train_epoch(heads),
   written out below; kind 3 is a fused pair launch.  The empty head is never paired: its actor and
   critic passes stay two launches.
2. The empty shard through the pipeline: train_epochs(heads, 2) with pairs on / off and one / two
   train streams trains bit-identical nets to two train_epoch calls; the empty head's gradients are
   zeroed, its parameters do not move (Adam on a zero gradient from zero moments) and its loss sums
   are 0."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

A, B, C = (13, 70), (13, 0), (20, 45)  # (n_in, local rows) of the three heads
EPOCHS_PAIRS = [(0, *A), (0, *B), (0, *C),
                (3, *A), (1, *B), (0, *B), (2, *C), (0, *C),
                (1, *A), (1, *B), (2, *C)]
EPOCHS_NO_PAIRS = [(0, *A), (0, *B), (0, *C),
                   (1, *A), (0, *A), (1, *B), (0, *B), (2, *C), (0, *C),
                   (1, *A), (1, *B), (2, *C)]
EPOCH = [(0, *A), (0, *B), (0, *C), (1, *A), (1, *B), (2, *C)]


def _heads():
    """The three heads, identically initialised at every call; the empty head's gradient buffers
    hold a sentinel the passes must zero."""
    from mhppo import ppo
    from mhppo.models import Model_PPO
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    heads = []
    for kind, (n_in, M), m in (("c", A, 70.0), ("c", B, 64.0), ("d", C, 45.0)):
        if kind == "c":
            actor = Model_PPO(n_in, 1, 1, mean=-1.0, std=3.0).to(dev)
            act = torch.from_numpy(rng.normal(-1, 1, M).astype(np.float32)).to(dev)
            counts = None
        else:
            actor = Model_PPO(n_in, 2, 2).to(dev)
            act = torch.from_numpy((rng.uniform(size=M) < 0.4).astype(np.int32)).to(dev)
            counts = torch.stack([(act == 0).sum(), (act == 1).sum()]).double()
        critic = Model_PPO(n_in, 1, 0).to(dev)
        obs = torch.from_numpy(rng.normal(0, 3, (M, n_in)).astype(np.float32)).to(dev)
        lp = torch.from_numpy(rng.normal(-0.6, 0.3, M).astype(np.float32)).to(dev)
        ret = torch.from_numpy(rng.normal(-20, 8, M).astype(np.float32)).to(dev)
        oa = torch.optim.Adam(actor.parameters(), 3e-4, fused=True)
        oc = torch.optim.Adam(critic.parameters(), 1e-3, fused=True)
        heads.append(ppo.Head(kind, actor, critic, oa, oc, obs, act, lp, ret, m, counts))
    for net in (heads[1].actor, heads[1].critic):
        net.grad_flat().fill_(1.0)
    return heads


def _flats(heads):
    return [n.flat().clone() for h in heads for n in (h.actor, h.critic)]


@pytest.mark.parametrize("driver,pairs,want", [("epochs", True, EPOCHS_PAIRS), ("epochs", False, EPOCHS_NO_PAIRS),
                                               ("epoch", True, EPOCH)], ids=["pairs", "no_pairs", "train_epoch"])
def test_launch_record(driver, pairs, want):
    from mhppo import ppo
    saved = ppo.TRAIN_EVENTS, ppo.TRAIN_STREAMS, ppo.PIPELINE_PAIRS
    heads = _heads()
    try:
        ppo.TRAIN_EVENTS, ppo.TRAIN_STREAMS, ppo.PIPELINE_PAIRS = [], 1, pairs
        if driver == "epochs":
            ppo.train_epochs(heads, 2)
        else:
            ppo.train_epoch(heads)
        torch.cuda.synchronize()
        events = ppo.TRAIN_EVENTS
    finally:
        ppo.TRAIN_EVENTS, ppo.TRAIN_STREAMS, ppo.PIPELINE_PAIRS = saved
    got = [tuple(e[:3]) for e in events]
    print(got)
    assert got == want
    assert all(e[3].elapsed_time(e[4]) >= 0.0 for e in events)


@pytest.fixture(scope="module")
def sequential():
    """Two train_epoch calls: (every net's flat weights, the initial ones)."""
    from mhppo import ppo
    heads = _heads()
    init = _flats(heads)
    for _ in range(2):
        ppo.train_epoch(heads)
    return _flats(heads), init


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("pairs", [True, False], ids=["pairs", "no_pairs"])
def test_empty_shard_through_the_pipeline(sequential, pairs, streams):
    from mhppo import ppo
    ref, init = sequential
    saved = ppo.TRAIN_STREAMS, ppo.PIPELINE_PAIRS
    heads = _heads()
    try:
        ppo.TRAIN_STREAMS, ppo.PIPELINE_PAIRS = streams, pairs
        losses = ppo.train_epochs(heads, 2)
        torch.cuda.synchronize()
    finally:
        ppo.TRAIN_STREAMS, ppo.PIPELINE_PAIRS = saved
    got = _flats(heads)
    for j, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"net {j} differs from two train_epoch calls"
    empty = heads[1]
    for j, net in ((2, empty.actor), (3, empty.critic)):
        assert not bool(net.grad_flat().any()), "the empty head's gradient is not zero"
        assert torch.equal(got[j].view(torch.int32), init[j].view(torch.int32)), "the empty head's net moved"
        assert torch.equal(ref[j].view(torch.int32), init[j].view(torch.int32))
    assert all(float(x) == 0.0 for x in losses[1])
    assert all(float(x) != 0.0 for k in (0, 2) for x in losses[k])
