"""External rollouts on the GPU (mhppo_record_begin / mhppo_record_step, mhppo.external, Algo_PPO
.train_external).  Every comparison is bit for bit:
  1. the two native launches against their torch specification (record_begin_torch / record_step_torch) on
     synthetic inputs between sentinel-filled guards, in both layouts, with NaN payloads and signed zeros;
  2. ExternalRollout.collect on a VecCrosswalk against RolloutGPU.collect on an identically seeded twin:
     the whole batch, then bucket_segments of both; native=False gives the same batch;
  3. Algo_PPO.train_external on a wrapped twin env against Algo_PPO.train: nets, Adam moments, curves;
  4. one training iteration on a torch "simulator" that is not a VecCrosswalk;
  5. misuse of the Python API and of the ABI."""
import ctypes

import numpy as np
import pytest
import torch

from test_policy_gpu import guarded, guards_intact, nets, same_bits

pytestmark = pytest.mark.gpu
SENT = -77.0
T3 = 3


def eq(a, b):
    return same_bits(a.cpu().numpy(), b.cpu().numpy())


# ------------------------------------------------------------------ 1. native vs spec
def synthetic(M, S, seed):
    """exist of density 0.5 with one stretch of absent segments, and a step's inputs per t < T3 with NaN
    payloads and -0.0 in act / logp / feat_c and NaN, -0.0 in the rewards"""
    NS = M * S
    g = torch.Generator().manual_seed(seed)
    exist = (torch.rand(NS, generator=g) < 0.5).to(torch.uint8)
    lo, n = (250, 300) if NS >= 600 else (NS // 4, NS // 2)
    exist[lo:lo + n] = 0
    if NS >= 600:
        assert not bool(exist[256:512].any())  # block 1 has no present segment
    if NS <= 2:
        exist[:] = 1
    steps = []
    for t in range(T3):
        x = {k: torch.randn(shape, generator=g) for k, shape in (("act", (M, S)), ("logp", (M, S)),
                                                                  ("feat_c", (M, S, 13)))}
        for k, v in x.items():
            flat = v.view(-1).view(torch.int32)
            idx = torch.randperm(flat.numel(), generator=g)
            flat[idx[:max(1, flat.numel() // 7)]] = 0x7FC12345 + t  # quiet NaNs with a payload
            flat[idx[-max(1, flat.numel() // 9):]] = -0x80000000     # -0.0
        rew = torch.randn((M, S), generator=g, dtype=torch.float64)
        rl = -torch.rand((M, S), generator=g, dtype=torch.float64) * (t + 1)
        pick = torch.randperm(NS, generator=g)
        rl.view(-1)[pick[:max(1, NS // 5)]] = float("nan")
        rl.view(-1)[pick[-max(1, NS // 6):]] = -0.0
        rew.view(-1)[pick[:max(1, NS // 8)]] = float("nan")
        steps.append({**{k: v.cuda() for k, v in x.items()}, "rew": rew.cuda(), "rew_light": rl.cuda()})
    return exist.reshape(M, S).cuda(), steps


@pytest.mark.parametrize("compact", [False, True], ids=["identity", "compact"])
@pytest.mark.parametrize("M,S", [(1, 1), (3, 2), (64, 4), (257, 3), (1031, 8)])
def test_native_equals_spec(M, S, compact):
    from mhppo import _lib
    from mhppo.external import record_begin_torch, record_step_torch
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    NS = M * S
    exist, steps = synthetic(M, S, 100 * M + S)
    if NS > 2:
        assert 0 < int(exist.sum()) < NS
    spec = dict(obs=(T3 * NS * 13, torch.float32), act=(T3 * NS, torch.float32), logp=(T3 * NS, torch.float32),
                rew=(T3 * NS, torch.float64), ep_min=(NS, torch.float64), rec=(NS + M + 1, torch.int32))
    bufs = {k: guarded(n, dt, int(SENT) if dt == torch.int32 else SENT) for k, (n, dt) in spec.items()}
    nat = {k: v[1] for k, v in bufs.items()}
    work = torch.empty(max(1, int(L.mhppo_record_work_bytes(M, S)) // 8), dtype=torch.float64, device="cuda")
    assert L.mhppo_record_begin(p(exist), M, S, p(nat["rec"]) if compact else None, p(nat["ep_min"]), p(work), st) == 0
    ep_ref, rec_ref = record_begin_torch(exist, compact)
    assert eq(nat["ep_min"].view(M, S), ep_ref)
    if compact:
        assert eq(nat["rec"], rec_ref)
    else:
        assert bool((nat["rec"] == int(SENT)).all())
    rec_of = nat["rec"][:NS] if compact else None
    ref = dict(obs=torch.full((T3, NS, 13), SENT, device="cuda"), act=torch.full((T3, NS), SENT, device="cuda"),
               logp=torch.full((T3, NS), SENT, device="cuda"),
               rew=torch.full((T3, NS), SENT, dtype=torch.float64, device="cuda"))
    for t, x in enumerate(steps):
        assert L.mhppo_record_step(M, S, t, T3, p(x["act"]), p(x["logp"]), p(x["feat_c"]), p(x["rew"]),
                                   p(x["rew_light"]), p(rec_of), p(nat["obs"]), p(nat["act"]), p(nat["logp"]),
                                   p(nat["rew"]), p(nat["ep_min"]), st) == 0
        record_step_torch(t, x["act"], x["logp"], x["feat_c"], x["rew"], x["rew_light"],
                          None if rec_of is None else rec_ref[:NS], ref["obs"], ref["act"], ref["logp"], ref["rew"], ep_ref)
        torch.cuda.synchronize()
        # the whole buffers: the steps not yet recorded and (compact) the absent records keep their sentinel
        for k in ("obs", "act", "logp", "rew"):
            assert eq(nat[k], ref[k].reshape(-1)), (t, k)
        assert eq(nat["ep_min"].view(M, S), ep_ref), t
    for k, (n, dt) in spec.items():
        assert guards_intact(bufs[k][0], n, int(SENT) if dt == torch.int32 else SENT), k
    if NS > 2:
        assert bool(torch.isnan(ep_ref).any()) and bool((ref["act"] == SENT).any()) == compact
    # the payloads and the signed zeros went through
    got = nat["act"].view(T3, NS)[0].view(torch.int32)
    src = steps[0]["act"].view(-1).view(torch.int32)
    keep = (rec_ref[:NS] >= 0) if compact else torch.ones(NS, dtype=torch.bool, device="cuda")
    assert same_bits(np.sort(got[:int(keep.sum())].cpu().numpy()), np.sort(src[keep].cpu().numpy()))
    if NS > 20:
        assert bool((src[keep] == 0x7FC12345).any()) and bool((src[keep] == -0x80000000).any())


def test_m_zero_touches_nothing():
    from mhppo import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    b = {k: torch.full((64,), SENT, dtype=dt, device="cuda") for k, dt in (
        ("f", torch.float32), ("d", torch.float64), ("i", torch.int32))}
    ex = torch.ones(64, dtype=torch.uint8, device="cuda")
    assert L.mhppo_record_work_bytes(0, 3) >= 0
    assert L.mhppo_record_begin(p(ex), 0, 3, p(b["i"]), p(b["d"]), p(b["d"]), st) == 0
    assert L.mhppo_record_step(0, 3, 0, 1, p(b["f"]), p(b["f"]), p(b["f"]), p(b["d"]), p(b["d"]), p(b["i"]), p(b["f"]),
                               p(b["f"]), p(b["f"]), p(b["d"]), p(b["d"]), st) == 0
    assert L.mhppo_record_step(0, 3, 0, 1, *([None] * 11), st) == 0
    torch.cuda.synchronize()
    assert all(bool((v == SENT).all()) for v in b.values())


# ------------------------------------------------------------------ 2. collector equivalence
COLLECT = [("coop", 4, 2, 2, 0, 80), ("naif", 1, 1, 1, 0, 80), ("4cars", 4, 1, 2, 0, 80), ("scalable", 4, 3, 2, 0, 80),
           ("scalable", 8, 2, 4, 0, 80), ("scalable", 8, 2, 4, 192, 80), ("coop", 2, 1, 2, 0, 7)]
BATCH_KEYS = ("a_d", "logp_d", "probs_d", "feat_d", "closest", "exist", "ep_min")
TM_KEYS = ("obs_c_tm", "act_tm", "logp_tm", "rew_tm")


def make_env(case, N=64):
    from mhppo.env import VecCrosswalk
    variant, nb_car, nb_ped, nb_lines, off, T = case
    return VecCrosswalk(variant, N, nb_car, nb_ped, nb_lines, max_episode=T, seed_base=900, env_id_offset=off)


def actors(dc, seed=5):
    from mhppo.models import Model_PPO
    torch.manual_seed(seed)
    return (Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda(), Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda(),
            Model_PPO(dc, 2, 2).cuda())


def buckets_equal(x, y):
    for name, a, b in zip(("cross", "wait", "choice"), x, y):
        assert set(a) == set(b), name
        for k in a:
            if k == "n_seg":
                assert a[k] == b[k], (name, k)
            else:
                assert eq(a[k], b[k]), (name, k)


@pytest.mark.parametrize("case", COLLECT, ids=lambda c: "%s_%d%d%d_off%d_T%d" % c)
def test_collect_equals_collector(case):
    from mhppo.external import ExternalRollout
    from mhppo.policy import Policy
    from mhppo.rollout import RolloutGPU, bucket_segments
    N, seed, iteration = 64, 4, 2
    off, T = case[4], case[5]
    venv = make_env(case)
    ro = RolloutGPU(venv)
    assert ro.T == T
    ac, aw, ad = actors(ro.dc)
    ref = ro.collect(ac, aw, ad, seed=seed, iteration=iteration)
    pol = Policy.from_env(venv, ac, aw, ad)
    got = {}
    for native in (True, False):
        ext = ExternalRollout(pol, N, T=T, seed=seed, first_env=off, native=native)
        assert ext.compact == ro.compact == (case[0] == "scalable")
        # a fresh twin: collect's sim.reset() is the reset mhppo_rollout_begin gives the collector's env
        got[native] = (ext, ext.collect(make_env(case), iteration))
    ext, b = got[True]
    assert (b.N, b.S, b.P, b.T) == (ref.N, ref.S, ref.P, ref.T)
    for k in BATCH_KEYS:
        assert eq(getattr(b, k), getattr(ref, k)), k
    present = ref.exist.reshape(-1).bool()
    if case[0] == "scalable":
        assert bool(present.any()) and not bool(present.all())
        assert eq(b.rec_of, ref.rec_of) and eq(ext.rec_buf, ro.rec_buf)
        for k in TM_KEYS:  # the whole buffers: nothing past the present segments' records on either side
            assert eq(getattr(b, k), getattr(ref, k)), k
    else:
        assert b.rec_of is None and ref.rec_of is None and bool(present.all())
        for k in TM_KEYS:
            x, y = (getattr(z, k).reshape(T, N * b.S, -1)[:, present] for z in (b, ref))
            assert eq(x, y), k
        for k in ("obs_c", "act", "logp", "rew"):  # the [env, slot, t] views
            assert eq(getattr(b, k), getattr(ref, k)) and getattr(b, k).shape[:3] == (N, b.S, T), k
    assert 0 < int(b.a_d.sum()) < b.a_d.numel()
    x = bucket_segments(b, status=ext.status)
    y = bucket_segments(ref, status=ro.status)
    assert 0 < x[0]["n_seg"] and 0 < x[1]["n_seg"]
    assert x[0]["obs"].shape[0] == x[0]["n_seg"] * T and x[2]["n_seg"] == int(present.sum())
    buckets_equal(x, y)
    assert "counts" in x[2] and "rew_sums" in x[2]
    # the torch specification of the record pass in the loop: the same batch
    ext2, b2 = got[False]
    for k in BATCH_KEYS + TM_KEYS:
        assert eq(getattr(b2, k), getattr(b, k)), k
    if b.rec_of is not None:
        assert eq(ext2.rec_buf, ext.rec_buf)


# ------------------------------------------------------------------ 3. training equivalence
class TwinSim:
    """A VecCrosswalk behind reset() / step(), given the resets Algo_PPO gives its own env: one at construction
    (Env_rollout.__init__), one before every episode (train()'s first rollout.reset()), the episode's own
    (mhppo_rollout_begin's), and one after every update (train()'s second rollout.reset())."""

    def __init__(self, env):
        self.env, self.played = env, False
        env.reset(want_obs=False)

    def reset(self):
        if self.played:
            self.env.reset(want_obs=False)
        self.played = True
        self.env.reset(want_obs=False)
        return self.env.reset()

    def step(self, actions):
        return self.env.step(actions)


def algo_state(a):
    out = {}
    for i, net in enumerate(a.nets()):
        for k, v in net.state_dict().items():
            out[f"net{i}.{k}"] = v
    for name, o in a._optimizers().items():
        for j, s in o.state_dict()["state"].items():
            for k, v in s.items():
                out[f"opt.{name}.{j}.{k}"] = v if torch.is_tensor(v) else torch.tensor(v)
    return out


@pytest.mark.parametrize("opts", [{}, dict(gae_lambda=0.95, max_grad_norm=0.5, minibatches=2, diagnostics=True)],
                         ids=["defaults", "gae_clip_minibatch_diag"])
@pytest.mark.parametrize("shape", [("scalable", 4, 3, 2), ("coop", 4, 2, 2)], ids=lambda s: "%s_%d%d%d" % s)
def test_train_external_equals_train(shape, opts):
    from mhppo.algo import Algo_PPO
    from mhppo.models import Model_PPO
    case = shape + (0, 80)
    torch.manual_seed(3)
    a = Algo_PPO(Model_PPO, make_env(case), seed=6, verbose=False, save_curves=False, **opts)
    b = Algo_PPO(Model_PPO, make_env(case), seed=6, verbose=False, save_curves=False, **opts)
    for na, nb in zip(a.nets(), b.nets()):
        nb.load_state_dict(na.state_dict())
    sim = TwinSim(make_env(case))
    before = {k: v.clone() for k, v in algo_state(a).items()}
    a.train(2)
    b.train_external(sim, 2, M=64)
    sa, sb = algo_state(a), algo_state(b)
    assert set(sa) == set(sb) and any(k.startswith("opt.") and k.endswith("exp_avg") for k in sa)
    for k in sa:
        assert eq(sa[k], sb[k]), k
    assert any(not eq(sa[k], before[k]) for k in before if k.startswith("net"))
    ca, cb = a.curves(), b.curves()
    assert ca == cb and len(ca[2]) == 2 and all(c + w > 0 for c, w in ca[3])
    assert a.rollout.iteration == b.rollout.iteration == 2 and a.total_loop == b.total_loop == 2
    if opts:
        assert repr(a.diagnostics) == repr(b.diagnostics) and len(a.diagnostics) == 2  # (repr: a NaN equals itself)
        assert repr(a.grad_norms) == repr(b.grad_norms) and len(a.grad_norms) == 2
    else:
        assert a.diagnostics == b.diagnostics == [] and a.grad_norms == b.grad_norms == []


# ------------------------------------------------------------------ 4. a foreign simulator
class TorchSim:
    """Not a VecCrosswalk: observation rows from a seeded generator, rewards a fixed function of the actions."""

    def __init__(self, M, obs_dim, S, seed=11):
        self.M, self.obs_dim, self.S = M, obs_dim, S
        self.g = torch.Generator(device="cuda").manual_seed(seed)
        self.steps = 0

    def rows(self):
        return torch.rand((self.M, self.obs_dim), generator=self.g, device="cuda") * 0.9 + 0.1

    def reset(self):
        return self.rows()

    def step(self, actions):
        self.steps += 1
        acc, light = actions[:, :self.S], actions[:, self.S:]
        return self.rows(), -0.1 * acc * acc, -(acc.abs() + 0.25 * (light + 1.0))


def test_foreign_simulator_trains():
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    M = 96
    venv = VecCrosswalk("coop", 1, 4, 2, 2, seed_base=1)
    torch.manual_seed(8)
    algo = Algo_PPO(Model_PPO, venv, seed=2, verbose=False, save_curves=False)
    S, T = venv.n_slots, venv.max_episode
    sim = TorchSim(M, venv.obs_dim, S)
    before = [p.detach().clone() for net in algo.nets() for p in net.parameters()]
    algo.train_external(sim, 1, M=M)
    torch.cuda.synchronize()
    after = [p.detach() for net in algo.nets() for p in net.parameters()]
    assert all(bool(torch.isfinite(p).all()) for p in after)
    assert any(not torch.equal(x, y) for x, y in zip(before, after))
    r = algo.rollout
    assert sim.steps == T and r.iteration == 1 and algo.total_loop == 1
    assert r.cross["n_seg"] + r.wait["n_seg"] == M * S == r.choice["n_seg"]
    for b in (r.cross, r.wait):
        assert b["obs"].shape == (b["n_seg"] * T, 13) and b["ret"].numel() == b["n_seg"] * T
    assert r.batch.N == M and len(algo.curves()[2]) == 1


# ------------------------------------------------------------------ 5. misuse
def test_api_rejects_misuse():
    from mhppo import _lib
    from mhppo.env import VecCrosswalk
    from mhppo.external import ExternalRollout
    from mhppo.models import Model_PPO
    from mhppo.policy import Policy
    from mhppo.rollout import bucket_segments
    ac, aw, ad = nets(17)
    pol = Policy("coop", 2, 1, 2, ac, aw, ad)
    M, S, T = 5, pol.n_slots, 3
    with pytest.raises(ValueError):
        ExternalRollout(pol, M, T=T, compact=True)  # the scalable variant's layout
    pol42 = Policy("4cars2", 2, 1, 2, ac, aw, Model_PPO(_dims42()[3], 2, 2).cuda())
    with pytest.raises(ValueError):
        ExternalRollout(pol42, M)  # an env-level variant only, as RolloutGPU has it
    ext = ExternalRollout(pol, M, T=T)
    obs = VecCrosswalk("coop", M, 2, 1, 2, seed_base=3).reset()
    rew = torch.zeros((M, S), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        ext.act(obs, 0)  # before begin
    with pytest.raises(ValueError):
        ext.begin(obs[:4], 0)  # one row per stream
    ext.begin(obs, 0)
    with pytest.raises(ValueError):
        ext.record(rew, rew)  # before act
    with pytest.raises(ValueError):
        ext.batch()
    with pytest.raises(ValueError):
        ext.act(obs, T)
    ext.act(obs, 1)
    with pytest.raises(ValueError):
        ext.record(rew, rew)  # step 1 before step 0
    ext.act(obs, 0)
    for bad in (rew[:4], rew.reshape(S, M), rew.cpu(), rew.reshape(-1), rew.long(), rew.bool(), [0.0] * M):
        with pytest.raises(ValueError):
            ext.record(bad, rew)
        with pytest.raises(ValueError):
            ext.record(rew, bad)
    ext.record(rew.float(), rew)  # float32 is converted
    with pytest.raises(ValueError):
        ext.record(rew, rew)  # twice for one step
    ext.act(obs, 2)
    with pytest.raises(ValueError):
        ext.record(rew, rew)  # step 2 after step 0
    with pytest.raises(ValueError):
        ext.batch()
    for t in (1, 2):
        ext.act(obs, t)
        ext.record(rew, rew)
    b = ext.batch()
    assert b.act.shape == (M, S, T) and b.rec_of is None and b.probs_d.shape == (M, S, 1, 2)
    bucket_segments(b, status=ext.status)
    # a NaN choice net: the status word makes the bucketing raise, as RolloutGPU.check does
    with torch.no_grad():
        ad.layer4.bias[0] = float("nan")
    ext.begin(obs, 1)
    for t in range(T):
        ext.act(obs, t)
        ext.record(rew, rew)
    with pytest.raises(_lib.MhppoNaNError):
        bucket_segments(ext.batch(), status=ext.status)
    assert int(ext.status.item()) == 0  # raised on and cleared


def _dims42():
    from mhppo import _lib
    from mhppo.env import VARIANTS
    cfg = _lib.EnvCfg()
    cfg.variant, cfg.n_envs, cfg.max_episode = VARIANTS["4cars2"], 1, 80
    cfg.nb_car, cfg.nb_ped, cfg.nb_lines, cfg.dt = 2, 1, 2, 0.3
    dims = (ctypes.c_int32 * 4)()
    if _lib.lib().mhppo_policy_dims(ctypes.byref(cfg), dims) != 0:
        raise ValueError("mhppo_policy_dims refuses 4cars2")
    return [int(x) for x in dims]


def test_abi_rejects_bad_input():
    from mhppo import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    M, S, T = 4, 2, 3
    NS = M * S
    f = lambda n: torch.full((n,), SENT, dtype=torch.float32, device="cuda")
    d = lambda n: torch.full((n,), SENT, dtype=torch.float64, device="cuda")
    src = dict(act=f(NS), logp=f(NS), feat_c=f(NS * 13), rew=d(NS), rew_light=d(NS))
    dst = dict(obs=f(T * NS * 13), act=f(T * NS), logp=f(T * NS), rew=d(T * NS), ep_min=d(NS))
    rec = torch.full((NS + M + 1,), int(SENT), dtype=torch.int32, device="cuda")
    ex = torch.ones(NS, dtype=torch.uint8, device="cuda")
    work = d(8)

    def step(M=M, S=S, t=0, T=T, **null):
        a = {**src, **{"d_" + k: v for k, v in dst.items()}}
        a = {k: (None if k in null else p(v)) for k, v in a.items()}
        return L.mhppo_record_step(M, S, t, T, a["act"], a["logp"], a["feat_c"], a["rew"], a["rew_light"], None,
                                   a["d_obs"], a["d_act"], a["d_logp"], a["d_rew"], a["d_ep_min"], st)

    def begin(M=M, S=S, e=ex, r=rec, m=dst["ep_min"], w=work):
        return L.mhppo_record_begin(p(e), M, S, p(r), p(m), p(w), st)

    bad = [step(t=-1), step(t=T), step(M=-1), step(S=0), step(M=2**30, S=2), step(M=2**31 - 1, S=2)]
    bad += [step(**{k: 1}) for k in list(src) + ["d_" + k for k in dst]]
    bad += [begin(M=-1), begin(S=0), begin(M=2**31, S=1), begin(m=None), begin(e=None), begin(w=None)]
    assert all(rc == -1 for rc in bad), bad
    assert L.mhppo_record_work_bytes(-1, 1) == -1 and L.mhppo_record_work_bytes(1, 0) == -1
    assert L.mhppo_record_work_bytes(2**30, 2) == -1 and L.mhppo_record_work_bytes(2**31 - 1, 1) > 0
    assert b"record" in L.mhppo_last_error()
    torch.cuda.synchronize()
    for v in list(dst.values()) + [work]:
        assert bool((v == SENT).all())
    assert bool((rec == int(SENT)).all())
    assert begin() == 0 and begin(r=None, e=None, w=None) == 0
    torch.cuda.synchronize()
    assert rec.tolist() == list(range(NS)) + [S * r for r in range(M + 1)] and bool((dst["ep_min"] == 0.0).all())
    assert step() == 0 and step(t=T - 1) == 0
    torch.cuda.synchronize()
    assert bool((dst["ep_min"] == SENT).all()) and bool((dst["act"].view(T, NS)[1] == SENT).all())
