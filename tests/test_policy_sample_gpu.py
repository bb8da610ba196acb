"""The stochastic policy on the GPU (mhppo_policy_sample_decide / _sample_act, mhppo.policy): bit for bit
the host build of the same rule (tools/hostpolicy.py, csrc/policy_sample_rule.h) on observation rows
harvested from the env, for the tape and for the in-kernel Philox noise; bit for bit the collector
(RolloutGPU.collect, which keeps its own statement of the rule) at t = 0 and in a closed loop over a whole
episode; the NaN flags; and the Python API's checks.

logp_d alone is compared with the host build at rtol = atol = 1e-5 (the device's logf against the host's,
the tolerance of tests/test_rollout_gpu.py); against the collector, whose k_choice calls the same device
logf, it is compared bit for bit.  The in-kernel normals are the device's Box-Muller (its logf / cosf, not
the host's: tests/test_noise_gpu.py bounds the difference), so the host build is run on the normals the
library's own Philox launch draws at the same counters, the launch the in-kernel draw replaces; the
uniforms are exact on both sides and the host build draws its own."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from test_policy_gpu import BIG, SIZES, guarded, guards_intact, harvest, nets, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu

SHAPES = [("coop", 2, 1, 2), ("naif", 1, 1, 1), ("scalable", 2, 2, 1), ("scalable", 4, 3, 2), ("scalable", 8, 2, 4),
          ("scalable", 8, 3, 4), ("4cars", 4, 1, 2)]
DEC_KEYS = ("a_d", "logp_d", "probs", "feat_d", "closest", "exist")
ACT_KEYS = ("actions", "act", "logp", "feat_c")
SEED, ITER, FIRST, STEP = 11, 3, 5, 2  # the Philox form's (seed, iteration), first_env and t


def noise_struct(tape=None, forced=None, key=0, first_env=0, t=0):
    from mhppo import _lib
    nz = _lib.PolicyNoise()
    nz.tape = None if tape is None else tape.data_ptr()
    nz.forced = None if forced is None else forced.data_ptr()
    nz.key, nz.first_env, nz.t = key, first_env, t
    return nz


def raw_decide(pol, obs, M, nz, full=True, status=None):
    """mhppo_policy_sample_decide on the first M rows, every output between sentinels (full=False: probs
    and feat_d NULL) -> dict of numpy"""
    from mhppo import _lib
    S, P, dc = pol.n_slots, pol.nb_ped, pol.choice_dim
    n = M * S * P
    spec = dict(a_d=(n, torch.int32, -77, (M, S, P)), logp_d=(n, torch.float32, -77.0, (M, S, P)),
                probs=(2 * n, torch.float32, -77.0, (M, S, P, 2)), feat_d=(n * dc, torch.float32, -77.0, (M, S, P, dc)),
                closest=(M * S, torch.int32, -77, (M, S)), exist=(M * S, torch.uint8, 171, (M, S)))
    if not full:
        del spec["probs"], spec["feat_d"]
    bufs = {k: guarded(v[0], v[1], v[2]) for k, v in spec.items()}
    p = lambda k: _lib.ptr(bufs[k][1]) if k in bufs else None
    d, keep = pol.actor_choice.mlp_desc()
    _lib.check(_lib.lib().mhppo_policy_sample_decide(ctypes.byref(pol.cfg), ctypes.byref(d), _lib.ptr(obs), M,
                                                     ctypes.byref(nz), p("a_d"), p("logp_d"), p("probs"), p("feat_d"),
                                                     p("closest"), p("exist"), _lib.ptr(status), _lib.stream_ptr()))
    torch.cuda.synchronize()
    for k, v in spec.items():
        assert guards_intact(bufs[k][0], v[0], v[2]), (M, k)
    return {k: bufs[k][1].cpu().numpy().reshape(v[3]) for k, v in spec.items()}


def raw_act(pol, obs, a_d, closest, M, nz, full=True, status=None):
    from mhppo import _lib
    S = pol.n_slots
    spec = dict(actions=(M * 2 * S, torch.float64, -77.0, (M, 2 * S)), act=(M * S, torch.float32, -77.0, (M, S)),
                logp=(M * S, torch.float32, -77.0, (M, S)), feat_c=(M * S * 13, torch.float32, -77.0, (M, S, 13)))
    if not full:
        del spec["feat_c"]
    bufs = {k: guarded(v[0], v[1], v[2]) for k, v in spec.items()}
    p = lambda k: _lib.ptr(bufs[k][1]) if k in bufs else None
    dc, kc = pol.actor_cross.mlp_desc()
    dw, kw = pol.actor_wait.mlp_desc()
    a_d, closest = a_d[:M].contiguous(), closest[:M].contiguous()
    _lib.check(_lib.lib().mhppo_policy_sample_act(ctypes.byref(pol.cfg), ctypes.byref(dc), ctypes.byref(dw),
                                                  _lib.ptr(obs), _lib.ptr(a_d), _lib.ptr(closest), M, ctypes.byref(nz),
                                                  p("actions"), p("act"), p("logp"), p("feat_c"), _lib.ptr(status),
                                                  _lib.stream_ptr()))
    torch.cuda.synchronize()
    for k, v in spec.items():
        assert guards_intact(bufs[k][0], v[0], v[2]), (M, k)
    return {k: bufs[k][1].cpu().numpy().reshape(v[3]) for k, v in spec.items()}


def check_decide(got, ref, M, what):
    for k in got:
        if k == "logp_d":
            np.testing.assert_allclose(got[k], ref[k][:M], rtol=1e-5, atol=1e-5, err_msg=str((M, what)))
        else:
            assert same_bits(got[k], ref[k][:M]), (M, what, k)


def device_normals(key, first_env, t, n, S):
    """The library's Philox normals at the collector's counters of step t for n rows from env first_env."""
    from mhppo import _lib
    out = torch.empty(n * S, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().mhppo_philox_normal(key, ((t + 1) << 40) + first_env * S, _lib.ptr(out), n * S,
                                              _lib.stream_ptr()))
    return out.view(n, S)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s_%d%d%d" % s)
def test_bits_equal_host_build(shape):
    import hostpolicy as hp
    from mhppo.models import Model_PPO
    from mhppo.policy import Policy, noise_key
    variant, nb_car, nb_ped, nb_lines = shape
    c = hp.cfg(variant, nb_car, nb_ped, nb_lines)
    od, S, P, dc = hp.dims(c)
    ac, aw, ad = nets(dc)
    torch.manual_seed(6)  # the second pair of continuous nets: mean 1, its candidates lie on both sides of 2.0
    hi = (Model_PPO(13, 1, 1, mean=1.0, std=3.0).cuda(), Model_PPO(13, 1, 1, mean=1.0, std=3.0).cuda())
    pols = {-1.0: Policy(variant, nb_car, nb_ped, nb_lines, ac, aw, ad),
            1.0: Policy(variant, nb_car, nb_ped, nb_lines, hi[0], hi[1], ad)}
    pol = pols[-1.0]
    sizes = SIZES + ([4099] if shape == BIG else [])
    top = max(sizes)
    obs = harvest(*shape)[:top].contiguous()
    o_np = obs.cpu().numpy()
    wd = ad.packed().cpu().numpy()
    wcont = {-1.0: [n.packed().cpu().numpy() for n in (ac, aw)], 1.0: [n.packed().cpu().numpy() for n in hi]}
    rng = np.random.default_rng(5)
    u = rng.uniform(size=(top, S, P)).astype(np.float32)
    eps = rng.normal(size=(top, S)).astype(np.float32)
    forced = rng.integers(0, 2, (top, S, P)).astype(np.int32)
    key = noise_key(SEED, ITER)
    eps_dev = device_normals(key, FIRST, STEP, top, S)

    # the host build, once, on all rows (a row's outputs depend on the row and its flat index alone)
    ref_dec = {"u": hp.sample_decide(c, wd, o_np, u=u), "forced": hp.sample_decide(c, wd, o_np, forced=forced),
               "philox": hp.sample_decide(c, wd, o_np, key=key, first_env=FIRST)}
    closest = ref_dec["u"]["closest"]
    sets = {"decided": ref_dec["u"]["a_d"], "cross": np.zeros_like(forced), "wait": np.ones_like(forced),
            "mixed": forced}
    runs = [(-1.0, k, "tape") for k in sets] + [(1.0, "decided", "tape"), (1.0, "mixed", "tape"),
                                                (-1.0, "decided", "philox"), (1.0, "mixed", "philox")]
    ref_act = {}
    for mean, k, form in runs:
        ref_act[mean, k, form] = hp.sample_act(c, *wcont[mean], o_np, sets[k], closest, mean=mean,
                                               eps=eps if form == "tape" else eps_dev.cpu().numpy())
    assert all(r["status"] == 0 for r in list(ref_dec.values()) + list(ref_act.values()))

    # what the compared rows must contain (conditions of the test, judged on the host build alone)
    assert 0 < ref_dec["u"]["a_d"].sum() < ref_dec["u"]["a_d"].size
    ped_there = np.ones((top, P), bool)
    if variant == "scalable":
        ped_there = o_np[:, od - 9 * P:].reshape(top, P, 9)[:, :, 7] != 0
        assert (~ped_there).any(), "no absent pedestrian harvested"
        assert (ref_dec["u"]["exist"] == 0).any(), "no absent car harvested"
    zero = np.zeros_like(eps)  # a = loc + L * 0: the fold's loc itself
    loc_hi = hp.sample_act(c, *wcont[1.0], o_np, sets["mixed"], closest, eps=zero, mean=1.0)["act"]
    assert ((loc_hi == 2.0) & ped_there.any(1)[:, None]).any(), "no slot whose every candidate exceeds 2.0"
    assert (loc_hi < 2.0).any()
    if P > 1:
        first = hp.features(c, o_np)[:, :, 0]
        assert any((r["feat_c"] != first).any() for r in ref_act.values()), "no slot with sel > 0"

    d_obs = {k: torch.from_numpy(v).cuda() for k, v in (("u", u), ("eps", eps), ("forced", forced))}
    d_sets = {k: torch.from_numpy(v).cuda() for k, v in sets.items()}
    d_closest = torch.from_numpy(closest).cuda()
    for M in sizes:
        check_decide(raw_decide(pol, obs, M, noise_struct(tape=d_obs["u"])), ref_dec["u"], M, "u")
        check_decide(raw_decide(pol, obs, M, noise_struct(forced=d_obs["forced"]), full=False), ref_dec["forced"], M,
                     "forced")
        check_decide(raw_decide(pol, obs, M, noise_struct(key=key, first_env=FIRST)), ref_dec["philox"], M, "philox")
        for mean, k, form in runs:
            nz = (noise_struct(tape=d_obs["eps"]) if form == "tape"
                  else noise_struct(key=key, first_env=FIRST, t=STEP))
            got = raw_act(pols[mean], obs, d_sets[k], d_closest, M, nz, full=(k != "cross"))
            for name in got:
                assert same_bits(got[name], ref_act[mean, k, form][name][:M]), (M, mean, k, form, name)

    # the Python API, and an obs view that starts 4 bytes off a 16-byte boundary
    M = 100
    shifted = torch.empty(M * od + 1, dtype=torch.float32, device="cuda")[1:].view(M, od)
    shifted.copy_(obs[:M])
    assert shifted.data_ptr() % 16 == 4
    for o in (obs[:M], shifted):
        d = pol.sample_decide(o, key=key, first_env=FIRST, want_probs=True, want_features=True)
        check_decide({k: getattr(d, k).cpu().numpy() for k in DEC_KEYS}, ref_dec["philox"], M, "api")
        d2 = pol.sample_decide(o, u=d_obs["u"][:M])
        assert d2.probs is None and d2.feat_d is None and same_bits(d2.a_d.cpu().numpy(), ref_dec["u"]["a_d"][:M])
        r = pol.sample_act(o, d2.a_d, d2.closest, key=key, first_env=FIRST, t=STEP)
        for name in ACT_KEYS:
            assert same_bits(getattr(r, name).cpu().numpy(), ref_act[-1.0, "decided", "philox"][name][:M]), name
        assert pol.sample_act(o, d2.a_d, d2.closest, eps=d_obs["eps"][:M], want_features=False).feat_c is None


def actors(dc, seed=5):
    from mhppo.models import Model_PPO
    torch.manual_seed(seed)
    return (Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda(), Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda(),
            Model_PPO(dc, 2, 2).cuda())


def collected(shape, N, off, seed, iteration):
    """(collector batch, policy, the reset observation of an identically seeded twin env, the twin)"""
    from mhppo.env import VecCrosswalk
    from mhppo.policy import Policy
    from mhppo.rollout import RolloutGPU
    venv = VecCrosswalk(*shape[:1], N, *shape[1:], seed_base=900, env_id_offset=off)
    twin = VecCrosswalk(*shape[:1], N, *shape[1:], seed_base=900, env_id_offset=off)
    ro = RolloutGPU(venv)
    ac, aw, ad = actors(ro.dc)
    obs0 = twin.reset()
    batch = ro.collect(ac, aw, ad, seed=seed, iteration=iteration)
    ro.check()
    return batch, Policy.from_env(venv, ac, aw, ad), obs0, twin, ro


def records(batch, name, t):
    """(step t's records of the present slots, the present-slot mask [N S]) in (env, slot) order"""
    x = getattr(batch, name + "_tm")[t]
    x = x.reshape(batch.N * batch.S, -1)
    if batch.rec_of is not None:  # the compact layout: present segments only, at their ranks
        m = batch.rec_of >= 0
        return x[batch.rec_of[m].long()], m
    m = batch.exist.reshape(-1).bool()
    return x[m], m


def eq(a, b):
    return same_bits(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("case", [("coop", 4, 2, 2, 0), ("4cars", 4, 1, 2, 0), ("scalable", 8, 2, 4, 0),
                                  ("scalable", 8, 2, 4, 192)], ids=lambda s: "%s_%d%d%d_off%d" % s)
def test_equals_collector_at_t0(case):
    from mhppo.policy import noise_key
    off, seed, iteration = case[4], 3, 2
    batch, pol, obs0, twin, ro = collected(case[:4], 64, off, seed, iteration)
    key = noise_key(seed, iteration)
    d = pol.sample_decide(obs0, key=key, first_env=off, want_probs=True, want_features=True)
    r = pol.sample_act(obs0, d.a_d, d.closest, key=key, first_env=off, t=0)
    assert eq(d.a_d, batch.a_d) and eq(d.logp_d, batch.logp_d) and eq(d.probs, batch.probs_d)
    assert eq(d.feat_d, batch.feat_d) and eq(d.closest, batch.closest) and eq(d.exist, batch.exist)
    assert 0 < int(d.a_d.sum()) < d.a_d.numel()
    act, m = records(batch, "act", 0)
    assert eq(m, d.exist.reshape(-1).bool())
    if case[0] == "scalable":
        assert not bool(m.all()) and bool(m.any())
    assert eq(r.act.reshape(-1, 1)[m], act)
    assert eq(r.logp.reshape(-1, 1)[m], records(batch, "logp", 0)[0])
    assert eq(r.feat_c.reshape(-1, 13)[m], records(batch, "obs_c", 0)[0])
    if off:  # the counters carry the global env id: first_env = 0 draws other noise
        assert not eq(pol.sample_decide(obs0, key=key, first_env=0).a_d, batch.a_d)


@pytest.mark.parametrize("shape", [("coop", 4, 2, 2), ("naif", 1, 1, 1), ("scalable", 4, 3, 2)],
                         ids=lambda s: "%s_%d%d%d" % s)
def test_closed_loop_equals_collector(shape):
    """A SamplingSession driving VecCrosswalk.step reproduces the collector's episode on an identically seeded env."""
    from mhppo.policy import SamplingSession
    N, seed, iteration = 64, 4, 1
    batch, pol, obs, twin, ro = collected(shape, N, 0, seed, iteration)
    sess = SamplingSession(pol, N, seed=seed)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d = sess.begin(obs, iteration, status=status)
    assert eq(d.a_d, batch.a_d)
    got = {k: [] for k in ("act", "logp", "obs_c", "rew")}
    for t in range(batch.T):
        actions = sess.step(obs, t, status=status)
        obs, rew = twin.step(actions)[:2]
        for k, v in (("act", sess.act), ("logp", sess.logp), ("obs_c", sess.feat_c), ("rew", rew)):
            got[k].append(v)
    assert int(status.item()) == 0
    for k, w in (("act", 1), ("logp", 1), ("obs_c", 13), ("rew", 1)):
        for t in range(batch.T):
            ref, m = records(batch, k, t)
            assert eq(got[k][t].reshape(N * batch.S, w)[m], ref), (k, t)


def test_nan_sets_status():
    from mhppo.policy import Policy
    ac, aw, ad = nets(17)
    pol = Policy("coop", 2, 1, 2, ac, aw, ad)
    obs = harvest("coop", 2, 1, 2)[:40].contiguous()
    u = torch.rand((40, 2, 1), device="cuda")
    eps = torch.randn((40, 2), device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d = pol.sample_decide(obs, u=u, status=status)
    pol.sample_act(obs, d.a_d, d.closest, eps=eps, status=status)
    assert int(status.item()) == 0
    with torch.no_grad():
        ad.layer4.bias[0] = float("nan")
    bad = pol.sample_decide(obs, u=u)  # status=None: nothing is written
    assert int(status.item()) == 0
    pol.sample_decide(obs, u=u, status=status)
    assert int(status.item()) == 1
    with torch.no_grad():
        aw.layer4.bias[0] = float("nan")
        ac.layer4.bias[0] = float("nan")
    r = pol.sample_act(obs, d.a_d, d.closest, eps=eps)
    assert int(status.item()) == 1 and bool(torch.isnan(r.act).all())
    pol.sample_act(obs, d.a_d, d.closest, eps=eps, status=status)
    assert int(status.item()) == 3 and bad.a_d.shape == (40, 2, 1)


def test_api_rejects_bad_input():
    from mhppo.models import Model_PPO
    from mhppo.policy import Policy, SamplingSession
    ac, aw, ad = nets(17)
    pol = Policy("coop", 2, 1, 2, ac, aw, ad)
    obs = torch.zeros((4, pol.obs_dim), device="cuda")
    u = torch.rand((4, 2, 1), device="cuda")
    eps = torch.randn((4, 2), device="cuda")
    d = pol.sample_decide(obs, u=u)
    assert d.a_d.shape == (4, 2, 1) and d.closest.shape == (4, 2) and d.exist.dtype == torch.uint8
    assert pol.sample_act(obs, d.a_d, d.closest, eps=eps).actions.shape == (4, 4)
    for kw in (dict(), dict(u=u, key=1), dict(u=u, forced=d.a_d), dict(forced=d.a_d, key=1)):
        with pytest.raises(ValueError):
            pol.sample_decide(obs, **kw)
    for kw in (dict(), dict(eps=eps, key=1)):
        with pytest.raises(ValueError):
            pol.sample_act(obs, d.a_d, d.closest, **kw)
    for bad in (d.closest.long(), d.closest[:3], d.closest.reshape(2, 4), d.closest.cpu()):
        with pytest.raises(ValueError):
            pol.sample_act(obs, d.a_d, bad, eps=eps)
    with pytest.raises(ValueError):
        pol.sample_act(obs, d.a_d.long(), d.closest, eps=eps)
    with pytest.raises(ValueError):
        pol.sample_decide(obs.cpu(), u=u)
    with pytest.raises(ValueError):
        pol.sample_act(obs.cpu(), d.a_d, d.closest, eps=eps)
    with pytest.raises(ValueError):
        pol.sample_decide(obs, u=u.double())
    with pytest.raises(ValueError):
        pol.sample_decide(obs, u=u, status=torch.zeros(1, device="cuda"))  # status is int32
    with pytest.raises(ValueError):
        pol.sample_act(obs, d.a_d, d.closest, key=1, t=-1)
    with pytest.raises(ValueError):
        Policy("coop", 2, 33, 2, ac, aw, Model_PPO(17, 2, 2).cuda())  # P > 32
    with pytest.raises(ValueError):
        SamplingSession(pol, 4).step(obs, 0)  # before begin
    with pytest.raises(ValueError):
        SamplingSession(pol, 5).begin(obs)  # one row per stream


def test_abi_rejects_bad_input():
    """The entry points' own checks, below the Python ones."""
    from mhppo import _lib
    from mhppo.policy import Policy
    ac, aw, ad = nets(17)
    pol = Policy("coop", 2, 1, 2, ac, aw, ad)
    L = _lib.lib()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    obs, u, eps = z((4, pol.obs_dim), torch.float32), z((4, 2, 1), torch.float32), z((4, 2), torch.float32)
    a_d, lp, cl, ex = z((4, 2, 1), torch.int32), z((4, 2, 1), torch.float32), z((4, 2), torch.int32), z((4, 2), torch.uint8)
    out, act, logp = z((4, 4), torch.float64), z((4, 2), torch.float32), z((4, 2), torch.float32)
    dc, _ = ac.mlp_desc()
    dw, _ = aw.mlp_desc()
    dd, _ = ad.mlp_desc()
    st, p, ref = _lib.stream_ptr(), _lib.ptr, ctypes.byref
    big_p = _lib.EnvCfg.from_buffer_copy(pol.cfg)
    big_p.nb_ped = 33
    tape, both = noise_struct(tape=u), noise_struct(tape=u, forced=a_d)

    def decide(cfg=pol.cfg, net=dd, o=obs, M=4, nz=tape, a=a_d):
        return L.mhppo_policy_sample_decide(ref(cfg), ref(net), p(o), M, ref(nz) if nz is not None else None, p(a),
                                            p(lp), None, None, p(cl), p(ex), None, st)

    def sact(cfg=pol.cfg, net=dc, o=obs, M=4, nz=noise_struct(tape=eps), c=cl):
        return L.mhppo_policy_sample_act(ref(cfg), ref(net), ref(dw), p(o), p(a_d), p(c), M,
                                         ref(nz) if nz is not None else None, p(out), p(act), p(logp), None, None, st)

    assert decide() == 0 and sact() == 0 and decide(M=0, o=None, a=None) == 0 and sact(M=0, o=None) == 0
    for rc in (decide(net=dc), decide(o=None), decide(a=None), decide(M=-1), decide(nz=None), decide(nz=both),
               sact(cfg=big_p), sact(net=dd), sact(o=None), sact(c=None), sact(M=-1), sact(nz=None),
               sact(nz=noise_struct(forced=a_d)), sact(nz=noise_struct(key=1, t=-1))):
        assert rc == -1
    assert sact(cfg=big_p) == -1 and b"nb_ped" in L.mhppo_last_error()
    torch.cuda.synchronize()
