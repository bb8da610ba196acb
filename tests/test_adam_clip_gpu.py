"""mhppo_adam_clip on the GPU (csrc/adam_clip.hip): the raw ABI against the specification
(mhppo.ppo.adam_clip_torch) bit for bit in p, m, v and step, the norms within one float64 ulp of
sqrt(ss); independence of the nets of a call, determinism, the first step, the ABI's edge cases;
then through Algo_PPO (max_grad_norm, grad_norms, knob off, resume)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import adam_clip_common as C
import fold_ref as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B1, B2, EPS = 0.9, 0.999, 1e-8


def _ragged8(n):
    """n elements as eight ragged segments that include a 1-element one (empty ones where n < 8 + ...)."""
    if n == 1:
        return [0, 1, 0, 0, 0, 0, 0, 0]
    cuts = sorted({0, 1, n} | {(n * k) // 11 for k in (2, 3, 5, 7, 10)} | {n // 2 + 1})
    cuts = (cuts + [n] * 9)[:9]
    cuts[8] = n
    segs = [b - a for a, b in zip(cuts, cuts[1:])]
    assert sum(segs) == n and len(segs) == 8 and 1 in segs and all(s >= 0 for s in segs)
    return segs


class Net:
    """One net's state as separate per-segment allocations, on the CPU (the specification's copy)
    and mirrored to the GPU; gradients per step from fold_ref.heavy scaled to `gscale`."""

    def __init__(self, segs, lr, gscale, seed, t0=0):
        self.segs, self.lr, self.gscale, self.t = list(segs), lr, gscale, t0
        self.rng = np.random.default_rng(seed)
        f = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))  # noqa: E731
        self.p = [f(0.1 * self.rng.standard_normal(s)) for s in segs]
        if t0:  # a state in mid-run
            self.m = [f(1e-3 * self.rng.standard_normal(s)) for s in segs]
            self.v = [f((1e-3 * self.rng.standard_normal(s)) ** 2) for s in segs]
        else:
            self.m = [torch.zeros(s) for s in segs]
            self.v = [torch.zeros(s) for s in segs]
        self.step = [torch.tensor(float(t0)) for _ in segs]
        self.g = [torch.zeros(s) for s in segs]
        self.dev = None

    def new_grad(self, poison=None):
        for g in self.g:
            g.copy_(torch.from_numpy((F.heavy(self.rng, g.numel()) * self.gscale).astype(np.float32)))
        if poison is not None:
            next(g for g in self.g if g.numel())[0] = poison

    def to_gpu(self):
        self.dev = [[x.to(DEV).clone() for x in xs] for xs in (self.p, self.g, self.m, self.v, self.step)]
        return self

    def push_grad(self):
        for d, g in zip(self.dev[1], self.g):
            d.copy_(g)

    def spec_step(self, max_norm, norm):
        from mhppo import ppo
        self.t += 1
        segs = list(zip(self.p, self.g, self.m, self.v, self.step))
        return ppo.adam_clip_torch(segs, self.t, self.lr, B1, B2, EPS, max_norm, norm=norm)

    def ss_norm(self):
        from mhppo import ppo
        return math.sqrt(float(ppo.adam_clip_sumsq(self.g)))

    def differs_from_gpu(self):
        """What differs in bits between the specification's copy and the GPU's: [] when nothing does."""
        out = []
        for name, host, dev in (("p", self.p, self.dev[0]), ("m", self.m, self.dev[2]), ("v", self.v, self.dev[3]),
                                ("step", self.step, self.dev[4])):
            for k, (h, d) in enumerate(zip(host, dev)):
                d = d.cpu()  # (a NaN equals a NaN: its sign and payload are not part of the contract)
                bad = int(((h.view(torch.int32) != d.view(torch.int32)) & ~(h.isnan() & d.isnan())).sum())
                if bad:
                    out.append(f"{name}[{k}]: {bad} of {h.numel()}")
        return out

    def snapshot(self):
        return [x.cpu().view(torch.int32).clone() for k in (0, 2, 3, 4) for x in self.dev[k]]


def _table(nets, ts):
    from mhppo import _lib
    tab = (_lib.AdamNet * max(1, len(nets)))()
    for e, net, t in zip(tab, nets, ts):
        e.n_seg = len(net.segs)
        for sg, p, g, m, v, st in zip(e.seg, *net.dev):
            sg.param, sg.grad, sg.exp_avg, sg.exp_avg_sq, sg.step = (x.data_ptr() for x in (p, g, m, v, st))
            sg.n = p.numel()
        e.t, e.alpha, e.bias2 = t, net.lr / (1.0 - B1 ** t), math.sqrt(1.0 - B2 ** t)
        e.beta1, e.beta2, e.eps = B1, B2, EPS
    return tab


def _launch(nets, max_norm, stream=None):
    """One mhppo_adam_clip call stepping `nets` (their GPU copies) from t to t + 1; returns the norms."""
    from mhppo import _lib
    norms = torch.full((len(nets),), math.nan, dtype=torch.float64, device=DEV)
    tab = _table(nets, [n.t + 1 for n in nets])
    s = stream if stream is not None else torch.cuda.current_stream(DEV)
    torch.cuda.synchronize()  # the inputs were written on the default stream
    with torch.cuda.device(DEV), torch.cuda.stream(s):
        _lib.adam_clip(tab, len(nets), max_norm, norms.data_ptr(), s.cuda_stream)
    s.synchronize()
    return norms.cpu()


def _run(nets, max_norm, steps=3):
    """`steps` calls with the state carried over, each checked against the specification fed with
    the kernel's norm; returns the (reference) norms [step][net]."""
    for n in nets:
        n.to_gpu()
    seen = []
    for _ in range(steps):
        for n in nets:
            n.new_grad()
            n.push_grad()
        got = _launch(nets, max_norm).tolist()
        row = []
        for n, x in zip(nets, got):
            want = n.ss_norm()
            assert abs(x - want) <= np.spacing(want), (x, want)
            n.spec_step(max_norm, x)
            assert n.differs_from_gpu() == []
            assert all(torch.equal(a, b.cpu()) for a, b in zip(n.g, n.dev[1]))  # grad is read, not written
            row.append(want)
        seen.append(row)
    return seen


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("n", F.EVS_N)
def test_single_net_sizes(n, ragged):
    segs = _ragged8(n) if ragged else [n]
    for max_norm, gscale in ((1.0, 1e-2), (1.0, 1e-9), (math.inf, 1e-2)):
        norms = _run([Net(segs, 1e-3, gscale, seed=n)], max_norm)
        if gscale == 1e-9:
            assert all(r[0] < 1.0 for r in norms)  # the unclipped case
        elif n >= 1023:
            assert any(r[0] > 1.0 for r in norms)  # the clipped one (or measured only, at inf)


@pytest.mark.parametrize("n_out", [1, 2])
@pytest.mark.parametrize("n_in", [1, 13, 54, 64])
def test_model_sizes(n_in, n_out):
    norms = _run([Net(C.model_segs(n_in, n_out), 3e-4, 1e-3, seed=n_in, t0=7),
                  Net(C.model_segs(n_in, n_out), 1e-3, 1e-9, seed=n_in + 100)], 0.5)
    assert all(r[0] > 0.5 and r[1] < 0.5 for r in norms)


def _six(gscales=(1e-9, 1e-2, 1e-3, 1e-9, 1e-2, 1e-8)):
    lrs = (3e-4, 2e-4, 1e-4, 1e-3, 2e-3, 5e-4)
    return [Net(C.model_segs(*s), lr, gs, seed=40 + k, t0=(k % 2) * 3)
            for k, (s, lr, gs) in enumerate(zip(C.PRODUCT_NETS, lrs, gscales))]


@pytest.mark.parametrize("which", [(0,), (0, 1), (0, 1, 2, 3, 4, 5), (0, 2, 3, 5)], ids=["1", "2", "6", "subset"])
@pytest.mark.parametrize("max_norm", [0.5, math.inf])
def test_calls_of_several_nets(which, max_norm):
    nets = [n for k, n in enumerate(_six()) if k in which]
    norms = _run(nets, max_norm)
    flat = [x for r in norms for x in r]
    if len(which) > 1:
        assert any(x > 0.5 for x in flat) and any(x < 0.5 for x in flat)


def test_nets_are_independent_and_the_call_is_deterministic():
    def fresh(which, poison=None):
        six = _six()
        nets = [six[k] for k in which]
        for n in nets:
            n.new_grad(poison=poison if n is nets[0] and poison is not None else None)
            n.to_gpu()
        return nets

    full = fresh(range(6))
    norms = _launch(full, 0.5)
    ref = {k: n.snapshot() for k, n in enumerate(full)}
    # the same call again, and on a side stream: the same bits
    for stream in (None, torch.cuda.Stream(DEV)):
        again = fresh(range(6))
        n2 = _launch(again, 0.5, stream)
        assert torch.equal(norms.view(torch.int64), n2.view(torch.int64))
        for k, n in enumerate(again):
            assert all(torch.equal(a, b) for a, b in zip(n.snapshot(), ref[k]))
    # a net's result does not depend on which other nets share the call
    for which in ((2,), (5, 2), (1, 2, 3)):
        part = fresh(which)
        n3 = _launch(part, 0.5)
        for j, k in enumerate(which):
            assert n3[j].view(torch.int64) == norms[k].view(torch.int64)
            assert all(torch.equal(a, b) for a, b in zip(part[j].snapshot(), ref[k]))
    # one inf gradient in net 0 poisons net 0 only
    bad = fresh(range(6), poison=math.inf)
    n4 = _launch(bad, 0.5)
    assert math.isinf(float(n4[0])) and torch.equal(n4[1:].view(torch.int64), norms[1:].view(torch.int64))
    for k in range(1, 6):
        assert all(torch.equal(a, b) for a, b in zip(bad[k].snapshot(), ref[k]))
    bad[0].spec_step(0.5, float(n4[0]))  # and net 0 itself follows the contract (s = 0: inf * 0 = NaN)
    assert bad[0].differs_from_gpu() == [] and not bool(torch.isfinite(bad[0].dev[0][0]).all())


def _gpu_nets():
    from mhppo.models import Model_PPO
    torch.manual_seed(3)
    nets = [Model_PPO(13, 1, 1, mean=-1.0, std=3.0).to(DEV), Model_PPO(13, 1, 0).to(DEV), Model_PPO(54, 2, 2).to(DEV)]
    lrs = (3e-4, 1e-3, 5e-4)
    return nets, [torch.optim.Adam(n.parameters(), lr, fused=True) for n, lr in zip(nets, lrs)], lrs


def test_first_step_goes_native(monkeypatch):
    from mhppo import _lib, ppo
    calls = []
    real = _lib.adam_clip
    monkeypatch.setattr(_lib, "adam_clip", lambda *a: (calls.append(a[1]), real(*a))[1])
    nets, opts, lrs = _gpu_nets()
    assert all(len(o.state) == 0 for o in opts)  # torch has created no Adam state yet
    rng = np.random.default_rng(5)
    ref_p = [n.flat().cpu().clone() for n in nets]
    ref_m = [torch.zeros_like(x) for x in ref_p]
    ref_v = [torch.zeros_like(x) for x in ref_p]
    for t in (1, 2):
        grads = [torch.from_numpy((F.heavy(rng, x.numel()) * sc).astype(np.float32)) for x, sc in
                 zip(ref_p, (1e-8, 1e-2, 1e-3))]
        for n, g in zip(nets, grads):
            n.grad_flat().copy_(g)
        norms = ppo.adam_steps(opts, max_grad_norm=0.5).cpu().tolist()
        assert calls == [3] * t  # one launch for the three optimisers, the first step included
        assert norms[0] < 0.5 < norms[1]
        for k, (n, o) in enumerate(zip(nets, opts)):
            step = torch.zeros(())
            ppo.adam_clip_torch([(ref_p[k], grads[k], ref_m[k], ref_v[k], step)], t, lrs[k], B1, B2, EPS, 0.5,
                                norm=norms[k])
            st = [o.state[p] for p in n.parameters()]
            assert torch.equal(n.flat().cpu().view(torch.int32), ref_p[k].view(torch.int32))
            assert torch.equal(torch.cat([s["exp_avg"].reshape(-1) for s in st]).cpu(), ref_m[k])
            assert torch.equal(torch.cat([s["exp_avg_sq"].reshape(-1) for s in st]).cpu(), ref_v[k])
            assert all(s["step"].device == n.flat().device and s["step"].dtype == torch.float32
                       and float(s["step"]) == t for s in st)
    for o in opts:  # torch's own step continues from the state the kernel keeps
        o.step()
    assert float(opts[0].state_dict()["state"][0]["step"]) == 3
    ppo.clip_forget(opts)


def test_abi_edge_cases():
    from mhppo import _lib
    L = _lib.lib()
    net = Net([5, 3], 1e-3, 1e-3, seed=1)
    net.new_grad()
    net.to_gpu()
    norms = torch.zeros(1, dtype=torch.float64, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream

    def call(tab, n, max_norm=1.0, nr=norms):
        return L.mhppo_adam_clip(ctypes.addressof(tab) if tab is not None else None, n, max_norm,
                                 nr.data_ptr() if nr is not None else None, st)

    before = net.snapshot()
    good = _table([net], [1])
    assert call(good, 0) == 0 and call(None, 0, 1.0, None) == 0  # n_nets == 0 launches nothing
    EINVAL = -1
    assert call(None, 1) == EINVAL and call(good, 1, 1.0, None) == EINVAL
    assert call(good, -1) == EINVAL and call((_lib.AdamNet * 9)(), _lib.ADAM_MAX_NETS + 1) == EINVAL
    for bad in (0.0, -1.0, math.nan, -math.inf):
        assert call(good, 1, bad) == EINVAL
    for field, val in (("beta1", 1.0), ("beta1", -0.1), ("beta2", 1.0), ("beta2", math.nan), ("n_seg", 9), ("n_seg", -1)):
        tab = _table([net], [1])
        setattr(tab[0], field, val)
        assert call(tab, 1) == EINVAL, field
    for field, val in (("n", -1), ("param", None), ("grad", None), ("exp_avg", None), ("exp_avg_sq", None),
                       ("step", None)):
        tab = _table([net], [1])
        setattr(tab[0].seg[1], field, val)
        assert call(tab, 1) == EINVAL, field
    assert b"adam_clip" in L.mhppo_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(net.snapshot(), before))  # a refused call touches nothing
    assert call(good, 1, math.inf) == 0  # and the table itself was fine
    torch.cuda.synchronize()
    assert float(net.dev[4][0]) == 1.0 and float(norms[0]) > 0.0


# ------------------------------------------------------------------ through the stack

def _algo(seed=5, **kw):
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    venv = VecCrosswalk("coop", 64, 2, 1, 2, seed_base=77)
    torch.manual_seed(seed)
    return Algo_PPO(Model_PPO, venv, verbose=False, save_curves=False, **kw)


def _net_bytes(algo):
    torch.cuda.synchronize()
    return [n.flat().cpu().view(torch.int32).clone() for n in algo.nets()]


_RUNS = {}


def _trained(clip):
    """(nets' bytes, grad_norms) of train(2) with max_grad_norm = clip, computed once."""
    if clip not in _RUNS:
        algo = _algo(max_grad_norm=clip)
        algo.train(2)
        algo.curves()
        _RUNS[clip] = (_net_bytes(algo), algo.grad_norms)
    return _RUNS[clip]


def _median_norm():
    _, gn = _trained(math.inf)
    allv = sorted(x for e in gn for k, v in e.items() if k != "iteration" for x in v)
    return allv, allv[len(allv) // 2]


def test_stack_records_norms_and_clips():
    nets_inf, gn_inf = _trained(math.inf)
    assert [e["iteration"] for e in gn_inf] == [0, 1]
    for e in gn_inf:
        keys = [k for k in e if k != "iteration"]
        assert keys and set(keys) <= {f"{a}_{h}" for a in ("actor", "critic") for h in ("cross", "wait", "choice")}
        assert {"actor_choice", "critic_choice"} <= set(keys)
        assert all(len(e[k]) == 10 and all(math.isfinite(x) and x >= 0.0 for x in e[k]) for k in keys)
    allv, c = _median_norm()
    assert allv[0] < c < allv[-1]  # norms on both sides of the bound
    nets_c, gn_c = _trained(c)
    assert any(not torch.equal(a, b) for a, b in zip(nets_inf, nets_c))  # clipping changed the run
    # before any step the gradients are the same: the first iteration's first-epoch norms agree
    for k in gn_inf[0]:
        if k != "iteration":
            assert gn_inf[0][k][0] == gn_c[0][k][0], k
    # the same run again: byte-identical nets and norms
    again = _algo(max_grad_norm=c)
    again.train(2)
    again.curves()
    assert all(torch.equal(a, b) for a, b in zip(_net_bytes(again), nets_c))
    assert again.grad_norms == gn_c


def test_knob_off_never_reaches_the_kernel(monkeypatch):
    from mhppo import _lib
    calls = []
    real = _lib.adam_clip
    monkeypatch.setattr(_lib, "adam_clip", lambda *a: (calls.append(1), real(*a))[1])
    algo = _algo()
    assert algo.max_grad_norm is None
    algo.train(2)
    algo.curves()
    assert calls == [] and algo.grad_norms == []
    on = _algo(max_grad_norm=math.inf)
    on.train(1)
    assert len(calls) == 11  # one launch per pipeline step


def test_resume_with_the_knob_set(tmp_path):
    _, c = _median_norm()
    nets_c, _ = _trained(c)
    a = _algo(max_grad_norm=c)
    a.train(1)
    a.save_checkpoint(str(tmp_path / "ck.pt"))
    b = _algo(seed=1234, max_grad_norm=c)
    b.load_checkpoint(str(tmp_path / "ck.pt"))
    b.train(1)
    assert all(torch.equal(x, y) for x, y in zip(_net_bytes(b), nets_c))
    assert b.grad_norms[0]["iteration"] == 1
