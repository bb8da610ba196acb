"""The KL early stop on the GPU (Algo_PPO(target_kl=tau)), layer by layer:
A. mhppo_ppo_kl / ppo.k_ppo_kl: the two sums carry the bits of mhppo_ppo_diag's DSUM and K3 (every case of
   test_infer_gpu.DIAG_CASES, and past one tile per wave on test_tile_walk_gpu's pools), the host terms'
   bars, streams, M == 0, the refusals;
B. mhppo_adam_clip_gated on the raw ABI: ungated and open nets carry mhppo_adam_clip's bits, a closed net
   keeps every bit (step included), the stop word is sticky and keeps the first epoch, the refusals;
C. ppo.train_epochs(target_kl=...): a head that stops at e has the actor of an e-epoch update and the
   critic of the full one, bit for bit (the oracle: reference runs with n_epochs = e), on every schedule;
D. Algo_PPO: kl_stops, determinism, resume, the knob off;
E. one rank with the data-parallel collectives forced on (RCCL) against the plain process.  Multi-rank
   RCCL has never run on this project's machines: it is NOT verified here.
The gate's decisions are held to the host specification (ppo.kl_gate, ppo.kl_limit) throughout."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adam_clip_common as C
import infer_common as ic
import test_adam_clip_gpu as tac
import test_infer_gpu as tig
import test_minibatch_gpu as tmb
import test_tile_walk_gpu as ttw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


# ------------------------------------------------------------------ A. the KL kernel
@pytest.mark.parametrize("akind,n_in,sigma,M,seed", tig.DIAG_CASES)
def test_kl_carries_the_diagnostics_bits(akind, n_in, sigma, M, seed):
    from mhppo import ppo
    c = ic.diag_case(akind, n_in, M, sigma, seed)
    h = tig.make_head(c)
    kl, dg = ppo.k_ppo_kl(h), ppo.k_ppo_diag(h)
    print(f"kl {kl.tolist()} diag {dg[:2].tolist()}")
    assert kl.shape == (2,) and kl.dtype == torch.float64
    assert torch.equal(_bits(kl), _bits(dg[:2]))
    # whatever critic the diagnostics call gets
    other = tig.make_head(c, Wc=c["Wc0"])
    assert torch.equal(_bits(kl), _bits(ppo.k_ppo_diag(other)[:2]))
    if M > 1:
        assert float(kl[1]) > 0.0  # the perturbed actor moved: not a comparison of zeros


@pytest.mark.parametrize("M", ttw.NET_MS[1:])
@pytest.mark.parametrize("akind,n_in,sigma,seed", ttw.DIAG_POOLS)
def test_kl_walk_carries_the_diagnostics_bits(akind, n_in, sigma, seed, M):
    """The second and third grid-stride steps: 65 537 and 131 239 rows (512 partials per term in the fold)."""
    from mhppo import _lib, ppo
    c, _ = ttw._diag_pool(akind, n_in, sigma, seed)
    h = tig.make_head(ttw._gathered(c, ttw.gather_idx(ttw.POOL_M, M)))
    assert _lib.lib().mhppo_ppo_kl_work_bytes(M) == 2 * 512 * 8
    kl, dg = ppo.k_ppo_kl(h), ppo.k_ppo_diag(h)
    assert torch.equal(_bits(kl), _bits(dg[:2])) and float(kl[1]) > 0.0


@pytest.mark.parametrize("akind,n_in,sigma,M,seed", [tig.DIAG_CASES[2], tig.DIAG_CASES[5]], ids=["kind1", "kind2"])
def test_kl_sums_vs_host_streams_and_repeat(akind, n_in, sigma, M, seed):
    """test_infer_gpu.test_diag_sums_vs_host's bars for the two sums (the bit identity above carries the rest
    of the cases), then the same bits on a second call, into a caller's tensor and on a side stream."""
    from mhppo import ppo
    c = ic.diag_case(akind, n_in, M, sigma, seed)
    d, terms, lp = ic.host_terms(c)
    h = tig.make_head(c)
    s1 = ppo.k_ppo_kl(h)
    got = s1.cpu().numpy()
    want, scale = terms.sum(0), np.abs(terms).sum(0)
    slack = 2.0 ** -22 * np.abs(lp.astype(np.float64)).sum() if akind == 2 else 0.0  # logf: <= 1 ulp each side
    for k in (ppo.DIAG_DSUM, ppo.DIAG_K3):
        print(f"term {k}: gpu {got[k]!r} host {want[k]!r} sum |term| {scale[k]:.3g}")
        assert abs(got[k] - want[k]) <= slack + 1e-10 * scale[k], k
    work = h._kl_work
    out = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    assert ppo.k_ppo_kl(h, out=out) is out and torch.equal(_bits(out), _bits(s1))
    assert h._kl_work is work  # the scratch is cached per head
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s3 = ppo.k_ppo_kl(h)
    side.synchronize()
    assert torch.equal(_bits(s1), _bits(s3))
    with pytest.raises(ValueError):
        ppo.k_ppo_kl(h, out=torch.zeros(2, device=DEV))  # not float64


def test_kl_einval_and_empty():
    from mhppo import _lib, ppo
    L = _lib.lib()
    c = ic.diag_case(1, 13, 8, 0.0, 77)
    h = tig.make_head(c)
    sums = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    work = torch.empty(64, dtype=torch.float64, device=DEV)
    p, st = _lib.ptr, _lib.stream_ptr()

    def kl(da, X=h.obs, act=h.act, lp=h.logp, s=sums, w=work, M=8):
        return L.mhppo_ppo_kl(ctypes.byref(da), p(X), M, p(act), p(lp), p(s), p(w), st)

    def desc(net, **kw):
        d, keep = net.mlp_desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    da = desc(h.actor)
    cases = [
        (lambda: kl(desc(h.critic)), "the actor is kind 0"),
        (lambda: kl(desc(h.actor, n_in=65)), "n_in 65"),
        (lambda: kl(desc(h.actor, n_in=0)), "n_in 0"),
        (lambda: kl(desc(h.actor, n_out=2)), "needs n_out 1"),
        (lambda: kl(desc(h.actor, kind=2)), "needs n_out 2"),
        (lambda: kl(desc(h.actor, packed=None)), "null pointer"),
        (lambda: kl(da, X=None), "null pointer"),
        (lambda: kl(da, act=None), "null pointer"),
        (lambda: kl(da, lp=None), "null pointer"),
        (lambda: kl(da, w=None), "null pointer"),
        (lambda: kl(da, s=None), "null pointer"),
        (lambda: kl(da, M=-1), "M < 0"),
    ]
    for call, msg in cases:
        with pytest.raises(_lib.MhppoError) as e:
            _lib.check(call())
        assert "error -1" in str(e.value) and msg in str(e.value), (msg, str(e.value))
    torch.cuda.synchronize()
    assert sums.tolist() == [7.0, 7.0]  # a refused call touches nothing
    assert kl(da) == 0
    torch.cuda.synchronize()
    assert sums.tolist() == [0.0, 0.0]  # d == 0 in every row: the unperturbed actor (sigma 0)
    # M == 0: two zeros, nothing else (the data pointers may be NULL)
    sums.fill_(7.0)
    assert kl(da, X=None, act=None, lp=None, w=None, M=0) == 0
    torch.cuda.synchronize()
    assert sums.tolist() == [0.0, 0.0]
    empty = ppo.Head("c", h.actor, h.critic, None, None, h.obs[:0], h.act[:0], h.logp[:0], h.ret[:0], 8)
    assert ppo.k_ppo_kl(empty).tolist() == [0.0, 0.0]
    with pytest.raises(ValueError):
        ppo.k_ppo_kl(ppo.Head("d", h.actor, h.critic, None, None, h.obs, h.act, h.logp, h.ret, 8))
    with pytest.raises(ValueError, match="GPU"):
        ppo.k_ppo_kl(ppo.Head("c", h.actor, h.critic, None, None, h.obs.cpu(), h.act.cpu(), h.logp.cpu(),
                              h.ret.cpu(), 8))


# ------------------------------------------------------------------ B. the gated step on the raw ABI
N_B = len(C.PRODUCT_NETS) + 1
LIMIT = 12.5


def _nets7():
    """The product's six nets and a one-element net, in mid-run (t0 = 7), with a gradient, on the GPU.
    Seeded: two calls give twins."""
    lrs = (3e-4, 2e-4, 1e-4, 1e-3, 2e-3, 5e-4)
    gss = (1e-9, 1e-2, 1e-3, 1e-9, 1e-2, 1e-8)
    nets = [tac.Net(C.model_segs(*s), lr, gs, seed=60 + k, t0=7) for k, (s, lr, gs) in
            enumerate(zip(C.PRODUCT_NETS, lrs, gss))]
    nets.append(tac.Net([1], 1e-3, 1e-2, seed=70, t0=7))
    for n in nets:
        n.new_grad()
        n.to_gpu()
    return nets


class _Gates:
    """Device KL sums and stop words for `n` nets, and the host gate table over them."""

    def __init__(self, n, kl1, gated=None, stop=None, epoch=3, limit=LIMIT):
        from mhppo import ppo
        self.kl = torch.tensor([[-0.25, x] for x in kl1], dtype=torch.float64, device=DEV)
        self.stop = torch.tensor(stop if stop is not None else [0] * n, dtype=torch.int32, device=DEV)
        self.gated = list(range(n)) if gated is None else list(gated)
        self.tab = ppo.gate_table([(self.kl[k].data_ptr(), limit, self.stop[k].data_ptr(), epoch)
                                   if k in self.gated else None for k in range(n)])

    def retable(self, epoch, limit=LIMIT):
        from mhppo import ppo
        n = self.kl.shape[0]
        self.tab = ppo.gate_table([(self.kl[k].data_ptr(), limit, self.stop[k].data_ptr(), epoch)
                                   if k in self.gated else None for k in range(n)])


def _call(nets, max_norm=0.5, gates="plain"):
    """One launch stepping `nets` from t to t + 1: mhppo_adam_clip ("plain") or mhppo_adam_clip_gated with
    `gates` (None: a NULL table).  Returns the norms' bits."""
    from mhppo import _lib
    norms = torch.full((len(nets),), -1.0, dtype=torch.float64, device=DEV)
    tab = tac._table(nets, [n.t + 1 for n in nets])
    torch.cuda.synchronize()
    st = torch.cuda.current_stream(DEV).cuda_stream
    with torch.cuda.device(DEV):
        if isinstance(gates, str):
            _lib.adam_clip(tab, len(nets), max_norm, norms.data_ptr(), st)
        else:
            _lib.adam_clip_gated(tab, len(nets), max_norm, norms.data_ptr(), None if gates is None else gates.tab, st)
    torch.cuda.synchronize()
    return norms.cpu()


def _same(snap_a, snap_b):
    return len(snap_a) == len(snap_b) and all(torch.equal(a, b) for a, b in zip(snap_a, snap_b))


@pytest.fixture(scope="module")
def plain7():
    """mhppo_adam_clip on the seven nets: (norms, per-net snapshots, the snapshots before the call)."""
    nets = _nets7()
    before = [n.snapshot() for n in nets]
    norms = _call(nets)
    after = [n.snapshot() for n in nets]
    assert all(not _same(a, b) for a, b in zip(before, after))  # every net stepped
    assert all(float(n.dev[4][0]) == 8.0 for n in nets)
    return norms, after, before


def test_gated_without_gates_is_adam_clip(plain7):
    norms, after, _ = plain7
    for gates in (None, _Gates(N_B, [0.0] * N_B, gated=[])):
        nets = _nets7()
        got = _call(nets, gates=gates)
        assert torch.equal(_bits(got), _bits(norms))
        assert all(_same(n.snapshot(), a) for n, a in zip(nets, after))
        if gates is not None:
            assert gates.stop.tolist() == [0] * N_B


def test_open_at_equality_steps_like_adam_clip(plain7):
    from mhppo import ppo
    norms, after, _ = plain7
    kl1 = [LIMIT, 0.0, math.nextafter(LIMIT, 0.0), LIMIT, 1e-300, LIMIT, LIMIT]
    assert all(ppo.kl_gate(x, LIMIT, 0, 3) == (True, 0) for x in kl1)
    g = _Gates(N_B, kl1)
    nets = _nets7()
    got = _call(nets, gates=g)
    assert torch.equal(_bits(got), _bits(norms))
    assert all(_same(n.snapshot(), a) for n, a in zip(nets, after))
    assert g.stop.tolist() == [0] * N_B
    # an infinite limit is open for every number
    g = _Gates(N_B, [1e300] * N_B, limit=math.inf)
    nets = _nets7()
    assert torch.equal(_bits(_call(nets, gates=g)), _bits(norms)) and g.stop.tolist() == [0] * N_B


@pytest.mark.parametrize("kl1", [math.nextafter(LIMIT, math.inf), 1e300, math.inf, math.nan],
                         ids=["just_above", "large", "inf", "nan"])
def test_closed_net_keeps_every_bit_and_the_stop_is_sticky(plain7, kl1):
    from mhppo import ppo
    _, _, before = plain7
    assert ppo.kl_gate(kl1, LIMIT, 0, 3) == (False, 3)
    g = _Gates(N_B, [kl1] * N_B, epoch=3)
    nets = _nets7()
    grads = [[x.clone() for x in n.dev[1]] for n in nets]
    got = _call(nets, gates=g)
    assert bool(got.isnan().all())  # "a net that was not stepped"
    assert all(_same(n.snapshot(), b) for n, b in zip(nets, before))  # p, m, v and step keep their bits
    assert all(float(n.dev[4][0]) == 7.0 for n in nets)
    assert g.stop.tolist() == [3] * N_B
    # a later call with a small KL and the next epoch: still closed, the first epoch kept
    g.kl[:, 1] = 0.0
    g.retable(epoch=4)
    assert ppo.kl_gate(0.0, LIMIT, 3, 4) == (False, 3)
    got = _call(nets, gates=g)
    assert bool(got.isnan().all())
    assert all(_same(n.snapshot(), b) for n, b in zip(nets, before))
    assert g.stop.tolist() == [3] * N_B
    assert all(torch.equal(a, b) for n, gs in zip(nets, grads) for a, b in zip(n.dev[1], gs))  # grad untouched


def test_six_nets_three_gated_one_closed(plain7):
    norms, after, before = plain7
    kl1 = [0.0] * N_B
    kl1[2] = LIMIT * 2  # the choice actor closes
    g = _Gates(N_B, kl1, gated=[0, 1, 2], epoch=5)
    nets = _nets7()[:6]  # (the table's first six entries serve the six nets)
    got = _call(nets, gates=g)
    for k in range(6):
        if k == 2:
            assert math.isnan(float(got[k])) and _same(nets[k].snapshot(), before[k])
        else:
            assert torch.equal(_bits(got[k:k + 1]), _bits(norms[k:k + 1])) and _same(nets[k].snapshot(), after[k])
    assert g.stop.tolist() == [0, 0, 5, 0, 0, 0, 0]


def test_gated_einval_touches_nothing(plain7):
    from mhppo import _lib, ppo
    L = _lib.lib()
    _, _, before = plain7
    nets = _nets7()
    g = _Gates(N_B, [LIMIT * 2] * N_B)  # every gate would close: a launch would show in stop and norms
    norms = torch.full((N_B,), -1.0, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream
    good = tac._table(nets, [8] * N_B)

    def call(tab=good, n=N_B, max_norm=0.5, nr=norms, gates=g.tab):
        return L.mhppo_adam_clip_gated(ctypes.addressof(tab) if tab is not None else None, n, max_norm,
                                       nr.data_ptr() if nr is not None else None,
                                       ctypes.addressof(gates) if gates is not None else None, st)

    def gates_with(k, **kw):
        ent = [(g.kl[j].data_ptr(), LIMIT, g.stop[j].data_ptr(), 3) for j in range(N_B)]
        tab = ppo.gate_table(ent)
        for name, v in kw.items():
            setattr(tab[k], name, v)
        return tab

    torch.cuda.synchronize()
    for what, rc in (("stop NULL", call(gates=gates_with(1, stop=None))),
                     ("epoch 0", call(gates=gates_with(2, epoch=0))),
                     ("epoch -1", call(gates=gates_with(6, epoch=-1))),
                     ("limit NaN", call(gates=gates_with(0, limit=math.nan))),
                     ("limit < 0", call(gates=gates_with(5, limit=-1e-300))),
                     ("limit -inf", call(gates=gates_with(5, limit=-math.inf))),
                     # everything mhppo_adam_clip refuses, with and without a gate table
                     ("nets NULL", call(tab=None)), ("norms NULL", call(nr=None)), ("n_nets -1", call(n=-1)),
                     ("n_nets 9", call(tab=(_lib.AdamNet * 9)(), n=9, gates=None)),
                     ("max_norm 0", call(max_norm=0.0)), ("max_norm NaN", call(max_norm=math.nan)),
                     ("max_norm 0, no gates", call(max_norm=0.0, gates=None))):
        assert rc == EINVAL, what
    assert b"adam_clip" in L.mhppo_last_error()
    for field, val in (("beta1", 1.0), ("beta2", math.nan), ("n_seg", 9)):
        tab = tac._table(nets, [8] * N_B)
        setattr(tab[3], field, val)
        assert call(tab=tab) == EINVAL, field
    tab = tac._table(nets, [8] * N_B)
    tab[4].seg[1].step = None
    assert call(tab=tab) == EINVAL
    torch.cuda.synchronize()
    assert all(_same(n.snapshot(), b) for n, b in zip(nets, before))
    assert g.stop.tolist() == [0] * N_B and norms.tolist() == [-1.0] * N_B
    # a gate that is not used (kl NULL) may carry anything; n_nets == 0 launches nothing
    assert call(gates=gates_with(1, kl=None, stop=None, epoch=0, limit=math.nan), n=0) == 0
    assert call(gates=g.tab) == 0  # and the table itself was fine: every gate closes
    torch.cuda.synchronize()
    assert g.stop.tolist() == [3] * N_B and bool(norms.isnan().all())
    assert all(_same(n.snapshot(), b) for n, b in zip(nets, before))


# ------------------------------------------------------------------ C. the pipeline
NAMES = tmb.NAMES
E = 10
_P = {}


def _buckets():
    if "buckets" not in _P:
        _P["buckets"] = tmb._collect(tmb._algo(0))
        rows = {n: _P["buckets"][n]["ret"].numel() for n in NAMES}
        print(f"rows per head: {rows}")
        assert all(r > 0 for r in rows.values())
    return _P["buckets"]


def _pipeline(n_epochs=E, clip=None, tau=None, calls=1, pairs=None, streams=1, forget_between=False, cache=True):
    """train_epochs on identically initialised nets over the one collected batch; returns a dict of the
    nets' and optimisers' state (tmb._state) and, per call, the driver's norms, kl and stop on the host."""
    from mhppo import ppo
    key = (n_epochs, clip, tau, calls, pairs, streams, forget_between)
    if cache and key in _P:
        return _P[key]
    a = tmb._algo(0)
    heads = tmb._heads(a, _buckets(), False)
    saved = ppo.TRAIN_STREAMS, ppo.PIPELINE_PAIRS
    out = {"norms": [], "kl": [], "stop": [], "m": [h.m for h in heads]}
    try:
        ppo.TRAIN_STREAMS, ppo.PIPELINE_PAIRS = streams, pairs
        for c in range(calls):
            if c and forget_between:
                ppo.clip_forget()
            if tau is None:
                res = ppo.train_epochs(heads, n_epochs, a.grad_bucket, clip)
                out["norms"].append(None if clip is None else res[1].cpu())
            else:
                _, norms, kl, stop = ppo.train_epochs(heads, n_epochs, a.grad_bucket, clip, tau)
                assert kl.shape == (n_epochs - 1, 3, 2) and kl.dtype == torch.float64 and kl.is_cuda
                assert stop.shape == (3,) and stop.dtype == torch.int32 and stop.is_cuda
                assert (norms is None) == (clip is None)
                out["norms"].append(None if norms is None else norms.cpu())
                out["kl"].append(kl.cpu())
                out["stop"].append(stop.cpu().tolist())
        torch.cuda.synchronize()
    finally:
        ppo.TRAIN_STREAMS, ppo.PIPELINE_PAIRS = saved
    out["state"] = tmb._state(a)
    out["actor_kl"] = [ppo.k_ppo_kl(h).cpu() for h in heads]  # of the nets as the run left them
    ppo.clip_forget()
    if cache:
        _P[key] = out
    return out


def _net_state(state, kind, name):
    return {k: v for k, v in state.items() if k.startswith(f"{kind}_{name}.")}


def _steps(state, kind, name):
    return {int(v) for k, v in _net_state(state, kind, name).items() if ".step" in k}


def _expected_stops(kl, ms, tau):
    """The stop of each head from an ungated trace, by the host specification: a head's trace equals the
    ungated one until it stops."""
    from mhppo import ppo
    stops = []
    for i, m in enumerate(ms):
        stop = 0
        for e in range(1, kl.shape[0] + 1):
            _, stop = ppo.kl_gate(float(kl[e - 1, i, 1]), ppo.kl_limit(tau, m), stop, e)
        stops.append(stop)
    return stops


def _pick_tau(kl, ms):
    """A tau under which some head stops at an epoch e in 2 .. E - 2: 1.5 tau halfway between that head's
    mean KL at e and the largest before it."""
    mean = [[float(kl[e - 1, i, 1]) / m for e in range(1, kl.shape[0] + 1)] for i, m in enumerate(ms)]
    for e in (4, 3, 5, 2, 6, 7, 8):
        for i, tr in enumerate(mean):
            before = max(tr[:e - 1])
            if tr[e - 1] > before * (1 + 1e-9) and before > 0.0:
                return (before + tr[e - 1]) / 2.0 / 1.5
    pytest.fail(f"no head's KL trace first exceeds its earlier values at an epoch in 2 .. {E - 2}: {mean}; "
                "change the seed or the shape of the batch")


def test_inf_measures_and_never_stops():
    from mhppo import ppo
    ref = _pipeline(clip=math.inf)
    got = _pipeline(clip=None, tau=math.inf)
    tmb._assert_same(got["state"], ref["state"])
    assert got["stop"][0] == [0, 0, 0] and got["norms"][0] is None
    kl = got["kl"][0]
    print("mean KL per epoch and head:", (kl[:, :, 1] / torch.tensor(got["m"])).tolist())
    assert bool(torch.isfinite(kl).all()) and bool((kl[..., 1] >= 0.0).all()) and bool((kl[..., 1] > 0.0).any())
    assert all(_steps(got["state"], k, n) == {E} for k in ("actor", "critic") for n in NAMES)
    # with the clip knob as well: the same nets, and the norms of the ungated run
    both = _pipeline(clip=math.inf, tau=math.inf)
    tmb._assert_same(both["state"], ref["state"])
    assert torch.equal(_bits(both["norms"][0]), _bits(ref["norms"][0]))
    assert torch.equal(_bits(both["kl"][0]), _bits(kl))
    # kl[e - 1] is the KL of the actors of an e-epoch update
    for e in (1, 4):
        short = _pipeline(n_epochs=e, clip=math.inf)
        for i in range(3):
            assert torch.equal(_bits(short["actor_kl"][i]), _bits(kl[e - 1, i])), (e, i)
    assert all(torch.equal(_bits(ref["actor_kl"][i]), _bits(got["actor_kl"][i])) for i in range(3))


def _check_stopped_run(got, tau, kl_inf, full):
    """`got` (a gated run) against the oracle: per head the actor of the n_epochs = stop reference run, the
    critic of the ungated full run, the step counts, and the kl rows after the stop."""
    want = _expected_stops(kl_inf, got["m"], tau)
    stop = got["stop"][0]
    print(f"tau {tau!r}: stops {stop}, expected {want}")
    assert stop == want
    kl = got["kl"][0]
    for i, name in enumerate(NAMES):
        s = stop[i] or E
        ref = full if s == E else _pipeline(n_epochs=s, clip=math.inf)
        tmb._assert_same(_net_state(got["state"], "actor", name), _net_state(ref["state"], "actor", name))
        tmb._assert_same(_net_state(got["state"], "critic", name), _net_state(full["state"], "critic", name))
        assert _steps(got["state"], "actor", name) == {s} and _steps(got["state"], "critic", name) == {E}
        assert torch.equal(_bits(kl[:s, i]), _bits(kl_inf[:s, i]))  # the ungated trace until the stop
        for e in range(s, E):  # the actor no longer moves: the stopping row repeats
            assert torch.equal(_bits(kl[e - 1, i]), _bits(kl[s - 1, i])), (name, e)
    return stop


def test_stop_is_the_e_epoch_actor_and_the_full_critic():
    full = _pipeline(clip=math.inf)
    kl_inf = _pipeline(tau=math.inf)["kl"][0]
    tau = _pick_tau(kl_inf, full["m"])
    stop = _check_stopped_run(_pipeline(tau=tau), tau, kl_inf, full)
    assert any(2 <= s <= E - 2 for s in stop), stop  # not vacuous
    # a tiny tau stops every head after its first step
    assert bool((kl_inf[0, :, 1] > 0.0).all())
    tiny = 1e-30
    assert _check_stopped_run(_pipeline(tau=tiny), tiny, kl_inf, full) == [1, 1, 1]


@pytest.mark.parametrize("pairs,streams", [(True, 1), (False, 1), (True, 2), (False, 2)])
def test_gated_run_on_every_schedule(pairs, streams):
    kl_inf = _pipeline(tau=math.inf)["kl"][0]
    tau = _pick_tau(kl_inf, _pipeline(clip=math.inf)["m"])
    ref = _pipeline(tau=tau)
    got = _pipeline(tau=tau, pairs=pairs, streams=streams, cache=False)
    tmb._assert_same(got["state"], ref["state"])
    assert got["stop"] == ref["stop"] and torch.equal(_bits(got["kl"][0]), _bits(ref["kl"][0]))


def test_two_gated_calls_keep_the_step_counts():
    kl_inf = _pipeline(tau=math.inf)["kl"][0]
    tau = _pick_tau(kl_inf, _pipeline(clip=math.inf)["m"])
    two = _pipeline(tau=tau, calls=2)
    twin = _pipeline(tau=tau, calls=2, forget_between=True)
    tmb._assert_same(two["state"], twin["state"])
    assert two["stop"] == twin["stop"] and any(two["stop"][0])  # the first call stopped a head
    assert two["stop"][0] == _pipeline(tau=tau)["stop"][0]
    for i, name in enumerate(NAMES):
        taken = sum(s[i] or E for s in two["stop"])
        assert _steps(two["state"], "actor", name) == {taken}, (name, two["stop"])
        assert _steps(two["state"], "critic", name) == {2 * E}


def test_gate_with_a_finite_clip():
    unclipped = _pipeline(clip=math.inf)["norms"][0]
    c = float(unclipped[torch.isfinite(unclipped)].median())
    clipped = _pipeline(clip=c)
    assert bool((clipped["norms"][0] > c).any()) and bool((clipped["norms"][0] < c).any())  # the clip is real
    trace = _pipeline(clip=c, tau=math.inf)
    tmb._assert_same(trace["state"], clipped["state"])
    tau = _pick_tau(trace["kl"][0], trace["m"])
    got = _pipeline(clip=c, tau=tau)
    stop = got["stop"][0]
    assert stop == _expected_stops(trace["kl"][0], got["m"], tau) and any(2 <= s <= E - 2 for s in stop)
    norms, ref, H = got["norms"][0], clipped["norms"][0], 3
    assert norms.shape == (E, 2 * H)
    for i in range(H):
        s = stop[i] or E
        assert torch.equal(_bits(norms[:, i]), _bits(ref[:, i]))            # the critic: every step, the same
        assert torch.equal(_bits(norms[:s, H + i]), _bits(ref[:s, H + i]))  # the actor up to its stop
        assert bool(norms[s:, H + i].isnan().all()) and bool(torch.isfinite(norms[:s, H + i]).all())


def test_train_epochs_refuses():
    from mhppo import ppo
    a = tmb._algo(0)
    heads = tmb._heads(a, _buckets(), False)
    for bad in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="target_kl"):
            ppo.train_epochs(heads, 2, a.grad_bucket, None, bad)
    h = heads[0]
    cpu = ppo.Head("c", h.actor, h.critic, h.opt_actor, h.opt_critic, h.obs.cpu(), h.act.cpu(), h.logp.cpu(),
                   h.ret.cpu(), h.m)
    with pytest.raises(ValueError, match="GPU"):
        ppo.train_epochs([cpu], 2, None, None, 0.01)


# ------------------------------------------------------------------ D. through Algo_PPO
TAU_D = 0.01
_RUNS = {}


def _trained(tau=TAU_D, **kw):
    key = (tau, tuple(sorted(kw.items())))
    if key not in _RUNS:
        algo = tac._algo(target_kl=tau, **kw)
        algo.train(2)
        algo.curves()
        _RUNS[key] = (tac._net_bytes(algo), algo.kl_stops, algo.grad_norms)
    return _RUNS[key]


def test_stack_records_kl_stops():
    nets, ks, gn = _trained()
    assert [e["iteration"] for e in ks] == [0, 1] and gn == []  # grad_norms is max_grad_norm's alone
    for e in ks:
        heads = [k for k in e if k != "iteration"]
        assert heads and set(heads) <= set(NAMES) and "choice" in heads
        for k in heads:
            assert set(e[k]) == {"actor_steps", "approx_kl"}
            assert isinstance(e[k]["actor_steps"], int) and 1 <= e[k]["actor_steps"] <= 10
            assert len(e[k]["approx_kl"]) == 9 and all(math.isfinite(x) and x >= 0.0 for x in e[k]["approx_kl"])
            s = e[k]["actor_steps"]
            # the record agrees with the rule: the first KL above 1.5 tau is the stop, none before it is
            above = [x > 1.5 * TAU_D for x in e[k]["approx_kl"]]
            assert not any(above[:s - 1]) and (s == 10 or above[s - 1]), (k, s, e[k]["approx_kl"])
    print("kl_stops:", ks)
    # the same run again: byte-identical nets and records
    again = tac._algo(target_kl=TAU_D)
    again.train(2)
    again.curves()
    assert all(torch.equal(a, b) for a, b in zip(tac._net_bytes(again), nets))
    assert again.kl_stops == ks
    # with the clip knob too: both records
    _, ks2, gn2 = _trained(max_grad_norm=math.inf)
    assert [e["iteration"] for e in gn2] == [0, 1] and ks2 == ks


def test_resume_with_target_kl(tmp_path):
    nets, ks, _ = _trained()
    a = tac._algo(target_kl=TAU_D)
    a.train(1)
    a.save_checkpoint(str(tmp_path / "ck.pt"))
    b = tac._algo(seed=1234, target_kl=TAU_D)
    b.load_checkpoint(str(tmp_path / "ck.pt"))
    b.train(1)
    b.curves()
    assert all(torch.equal(x, y) for x, y in zip(tac._net_bytes(b), nets))
    assert b.kl_stops == ks[1:]  # not checkpointed: the resumed run starts empty


def test_knob_off_never_reaches_the_kl_path(monkeypatch):
    from mhppo import _lib, ppo

    def boom(*a, **k):
        raise AssertionError("the KL early stop was reached with target_kl=None")

    monkeypatch.setattr(_lib, "adam_clip_gated", boom)
    monkeypatch.setattr(_lib, "ppo_kl", boom)
    monkeypatch.setattr(ppo, "k_ppo_kl", boom)
    for kw in ({}, {"max_grad_norm": math.inf}, {"diagnostics": True}):
        algo = tac._algo(**kw)
        assert algo.target_kl is None
        algo.train(1)
        algo.curves()
        assert algo.kl_stops == [] and not algo._pending_kl
    monkeypatch.undo()
    calls = []
    real_gated, real_kl = _lib.adam_clip_gated, _lib.ppo_kl
    monkeypatch.setattr(_lib, "adam_clip_gated", lambda *a: (calls.append("adam"), real_gated(*a))[1])
    monkeypatch.setattr(_lib, "ppo_kl", lambda *a: (calls.append("kl"), real_kl(*a))[1])
    on = tac._algo(target_kl=math.inf)
    on.train(1)
    on.curves()
    H = len([k for k in on.kl_stops[0] if k != "iteration"])
    assert calls.count("adam") == 11 and calls.count("kl") == 9 * H  # one Adam launch per step, nine KL per head


# ------------------------------------------------------------------ E. data parallel, one rank
def test_rccl_one_rank_equals_the_plain_process(tmp_path):
    """One rank on RCCL with the collectives forced on (a one-rank SUM is the identity): the KL sums ride in
    the advantage-sum all-reduce and are reduced alone at the last step; nets and kl_stops carry the plain
    process's bits.  More than one rank on RCCL is not verified (never run on this project's machines)."""
    worker = os.path.join(ROOT, "tests", "target_kl_worker.py")
    env = dict(os.environ, OMP_NUM_THREADS="4")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    outs = []
    for name, extra in (("one", []), ("rccl", ["--nccl-world1"])):
        base = str(tmp_path / name)
        subprocess.run([sys.executable, worker, "--out", base] + extra, check=True, timeout=240, env=env, cwd=tmp_path)
        outs.append((np.load(base + ".npy"), json.load(open(base + ".json"))))
    (a, ka), (b, kb) = outs
    assert np.isfinite(a).all() and a.shape == b.shape
    assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert ka == kb and [e["iteration"] for e in ka["kl_stops"]] == [0, 1]
    steps = [e[k]["actor_steps"] for e in ka["kl_stops"] for k in e if k != "iteration"]
    print("tau", ka["tau"], "actor steps", steps)
    assert any(s < 10 for s in steps)  # the gate closed somewhere: the reduced sums decided
