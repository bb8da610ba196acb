"""The stateless policy on the GPU (mhppo_policy_decide / mhppo_policy_act, mhppo.policy): bit for bit
the host build of the same rule (tools/hostpolicy.py, csrc/policy_rule.h) on observation rows
harvested from the env; in a closed loop bit for bit RolloutGPU.evaluate (mhppo_eval_step, which
keeps its own statement of the rule); and the Python API's checks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
pytestmark = pytest.mark.gpu

# (variant, nb_car, nb_ped, nb_lines): P = 3 pads the act tile's groups, scalable x/x/4 has S = 8
# (choice_dim 54, the widest a shape here has), 4cars2 has S = 2 nb_car
SHAPES = [("coop", 2, 1, 2), ("naif", 1, 1, 1), ("scalable", 2, 2, 1), ("scalable", 4, 3, 2), ("scalable", 8, 2, 4),
          ("scalable", 8, 3, 4), ("4cars", 4, 1, 2), ("4cars2", 2, 1, 2)]
SIZES = [0, 1, 31, 32, 33, 100]
BIG = ("scalable", 8, 2, 4)  # + M = 4099: 65 584 triples = 2 050 decide tiles, past the 2 048 wave slots
N_ENVS, N_STEPS, SEED = 64, 70, 20
PAD = 64  # sentinel elements on either side of an output


def harvest(variant, nb_car, nb_ped, nb_lines):
    """Observation rows of 64 envs: the reset's and those after N_STEPS - 1 random-action steps,
    [N_STEPS * 64, obs_dim] in a fixed shuffled order (so that a prefix mixes early and late rows)."""
    from mhppo.env import VecCrosswalk
    venv = VecCrosswalk(variant, N_ENVS, nb_car, nb_ped, nb_lines, seed_base=SEED)
    S = venv.n_slots
    rng = np.random.default_rng(SEED)
    rows = [venv.reset()]
    for _ in range(N_STEPS - 1):
        # accelerations biased upwards: cars near the speed limit, where the (10 - V) / dt cap binds
        a = np.concatenate([rng.uniform(-1.5, 2, (N_ENVS, S)), rng.choice([-1.0, 1.0], (N_ENVS, S))], 1)
        rows.append(venv.step(torch.from_numpy(a).cuda())[0])
    obs = torch.cat(rows)
    perm = torch.from_numpy(np.random.default_rng(SEED + 1).permutation(len(obs))).cuda()
    return obs[perm].contiguous()


def nets(dc, seed=7):
    from mhppo.models import Model_PPO
    torch.manual_seed(seed)
    return (Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda(), Model_PPO(13, 1, 1, mean=-1.0, std=3.0).cuda(),
            Model_PPO(dc, 2, 2).cuda())


def guarded(n, dtype, fill):
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n]


def guards_intact(buf, n, fill):
    return bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all())


def raw_decide(pol, obs, M):
    """mhppo_policy_decide on the first M rows, outputs between sentinels: (a_d, probs) as numpy"""
    from mhppo import _lib
    S, P = pol.n_slots, pol.nb_ped
    n = M * S * P
    ab, a = guarded(n, torch.int32, -77)
    pb, pr = guarded(2 * n, torch.float32, -77.0)
    d, keep = pol.actor_choice.mlp_desc()
    _lib.check(_lib.lib().mhppo_policy_decide(ctypes.byref(pol.cfg), ctypes.byref(d), _lib.ptr(obs), M, _lib.ptr(a),
                                              _lib.ptr(pr), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(ab, n, -77) and guards_intact(pb, 2 * n, -77.0)
    return a.cpu().numpy().reshape(M, S, P), pr.cpu().numpy().reshape(M, S, P, 2)


def raw_act(pol, obs, a_d, M):
    from mhppo import _lib
    S = pol.n_slots
    ob, out = guarded(M * 2 * S, torch.float64, -77.0)
    dc, kc = pol.actor_cross.mlp_desc()
    dw, kw = pol.actor_wait.mlp_desc()
    a_d = a_d[:M].contiguous()
    _lib.check(_lib.lib().mhppo_policy_act(ctypes.byref(pol.cfg), ctypes.byref(dc), ctypes.byref(dw), _lib.ptr(obs),
                                           _lib.ptr(a_d), M, _lib.ptr(out), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(ob, M * 2 * S, -77.0)
    return out.cpu().numpy().reshape(M, 2 * S)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s_%d%d%d" % s)
def test_bits_equal_host_build(shape):
    import hostpolicy as hp
    from mhppo.policy import Policy
    variant, nb_car, nb_ped, nb_lines = shape
    c = hp.cfg(variant, nb_car, nb_ped, nb_lines)
    od, S, P, dc = hp.dims(c)
    ac, aw, ad = nets(dc)
    pol = Policy(variant, nb_car, nb_ped, nb_lines, ac, aw, ad)
    assert (pol.obs_dim, pol.n_slots, pol.nb_ped, pol.choice_dim) == (od, S, P, dc)
    obs = harvest(*shape)
    sizes = SIZES + ([4099] if shape == BIG else [])
    top = max(sizes)
    obs = obs[:top].contiguous()
    o_np = obs.cpu().numpy()
    wc, ww, wd = (n.packed().cpu().numpy() for n in (ac, aw, ad))

    # the rows exercise the rule's branches: a left-lane pedestrian and a capped action among the first 100
    f = hp.features(c, o_np[:100])
    assert (f[..., 7] != 0).any(), "no left-lane row harvested"
    ref_a, ref_p = hp.decide(c, wd, o_np, probs=True)
    rng = np.random.default_rng(5)
    sets = {"decided": ref_a, "cross": np.zeros_like(ref_a), "wait": np.ones_like(ref_a),
            "mixed": rng.integers(0, 2, ref_a.shape).astype(np.int32)}
    ref_act = {k: hp.act(c, wc, ww, o_np, v) for k, v in sets.items()}
    cap = (10.0 - f[..., 0].astype(np.float64)) / 0.3  # [100, S, P]
    capped = (ref_act["decided"][:100, :S, None] == cap) & (f[..., 7] == 0)
    assert capped.any(), "no capped row harvested"

    for M in sizes:
        a, p = raw_decide(pol, obs, M)
        assert same_bits(a, ref_a[:M]), (M, "a_d")
        assert same_bits(p, ref_p[:M]), (M, "probs")
        for k, v in sets.items():
            out = raw_act(pol, obs, torch.from_numpy(v).cuda(), M)
            assert same_bits(out, ref_act[k][:M]), (M, k)

    # the Python API, and an obs view that starts 4 bytes off a 16-byte boundary
    M = 100
    shifted = torch.empty(M * od + 1, dtype=torch.float32, device="cuda")[1:].view(M, od)
    shifted.copy_(obs[:M])
    assert shifted.data_ptr() % 16 == 4
    for o in (obs[:M], shifted):
        a, p = pol.decide(o, probs=True)
        assert same_bits(a.cpu().numpy(), ref_a[:M]) and same_bits(p.cpu().numpy(), ref_p[:M])
        assert same_bits(pol.decide(o).cpu().numpy(), ref_a[:M])
        assert same_bits(pol.act(o, a).cpu().numpy(), ref_act["decided"][:M])


@pytest.mark.parametrize("name", ["coop_212", "scalable_221"])
def test_closed_loop_equals_evaluate(name):
    """PolicySession driving VecCrosswalk.step reproduces RolloutGPU.evaluate on an identically seeded env."""
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    from mhppo.policy import Policy, PolicySession
    from mhppo.rollout import RolloutGPU
    g = np.load(os.path.join(ROOT, "tests", "golden", f"eval_{name}.npz"))
    variant, shape = str(g["variant"]), (int(g["nb_car"]), int(g["nb_ped"]), int(g["nb_lines"]))
    N, K, T = 4, 2, 80
    ac = Model_PPO(13, 1, 1, mean=-1.0, std=3.0).load_packed(g["w_cross"]).cuda()
    aw = Model_PPO(13, 1, 1, mean=-1.0, std=3.0).load_packed(g["w_wait"]).cuda()
    ad = Model_PPO((g["w_choice"].size - 4290) // 32, 2, 2).load_packed(g["w_choice"]).cuda()  # 32 dc + 4290 floats
    ref_env = VecCrosswalk(variant, N, *shape, seed_base=int(g["seed_base"]))
    ref = RolloutGPU(ref_env).evaluate(ac, aw, ad, K)
    venv = VecCrosswalk(variant, N, *shape, seed_base=int(g["seed_base"]), generic_step=True)
    pol = Policy.from_env(venv, ac, aw, ad)
    S = pol.n_slots
    sess = PolicySession(pol, N)
    obs_h, act_h = [], []
    for k in range(K):
        obs = venv.reset()
        for t in range(T):
            actions = sess.step(obs, start=True if t == 0 else None)
            obs_h.append(obs)
            act_h.append(actions[:, :S].float())
            obs = venv.step(actions)[0]
    # [K T, N, ..] -> env-major [N K T, ..]
    obs_h = torch.stack(obs_h).view(K, T, N, -1).permute(2, 0, 1, 3).reshape(N * K * T, -1)
    act_h = torch.stack(act_h).view(K, T, N, S).permute(2, 0, 1, 3).reshape(N * K * T, S)
    assert same_bits(obs_h.cpu().numpy(), ref[0].cpu().numpy())
    assert same_bits(act_h.cpu().numpy(), ref[1].cpu().numpy())


def test_algo_policy_tracks_weights():
    from mhppo.algo import Algo_PPO
    from mhppo.env import VecCrosswalk
    from mhppo.models import Model_PPO
    venv = VecCrosswalk("coop", 8, 2, 1, 2, seed_base=3)
    algo = Algo_PPO(Model_PPO, venv, verbose=False)
    pol = algo.policy()
    venv.reset()
    brake = torch.tensor([[-3.0, -3.0, -1.0, -1.0]], dtype=torch.float64, device="cuda").expand(8, 4)
    for _ in range(5):  # off the speed limit, where the (10 - V) / dt cap (0 at the reset) hides the heads
        obs = venv.step(brake)[0]
    a_d = torch.zeros((8, 2, 1), dtype=torch.int32, device="cuda")
    before = pol.act(obs, a_d)
    assert (before[:, :2] < 0.9 * (10.0 - obs[:, [1, 7]].double()) / 0.3).any()  # a head's action, not the cap
    with torch.no_grad():
        algo.actor_net_cross.layer4.bias += 0.5
    after = pol.act(obs, a_d)
    fresh = algo.policy().act(obs, a_d)
    assert not torch.equal(before, after) and torch.equal(after, fresh)


def test_api_rejects_bad_input():
    from mhppo._lib import MhppoError
    from mhppo.models import Model_PPO
    from mhppo.policy import Policy
    ac, aw, ad = nets(17)  # coop 2/1/2: choice_dim 2 + 5 + 10
    pol = Policy("coop", 2, 1, 2, ac, aw, ad)
    obs = torch.zeros((4, pol.obs_dim), device="cuda")
    a_d = pol.decide(obs)
    assert a_d.shape == (4, 2, 1) and pol.act(obs, a_d).shape == (4, 4)
    with pytest.raises(ValueError):
        pol.decide(torch.zeros((4, pol.obs_dim + 1), device="cuda"))  # wrong width
    with pytest.raises(ValueError):
        pol.decide(obs.cpu())  # no CPU path
    with pytest.raises(ValueError):
        pol.act(obs.cpu(), a_d)
    with pytest.raises(ValueError):
        pol.act(obs, a_d.long())
    with pytest.raises(ValueError):
        Policy("coop", 2, 1, 2, ac, aw, Model_PPO(18, 2, 2).cuda())  # the choice net's n_in
    with pytest.raises(ValueError):
        Policy("coop", 2, 1, 2, Model_PPO(13, 1, 0).cuda(), aw, ad)  # a critic as an actor
    with pytest.raises(ValueError):
        Policy("coop", 2, 33, 2, ac, aw, Model_PPO(17, 2, 2).cuda())  # P > 32
    with pytest.raises((ValueError, MhppoError)):
        Policy("no_such_variant", 2, 1, 2, ac, aw, ad)
    with pytest.raises((ValueError, MhppoError)):
        Policy("coop", 17, 1, 2, ac, aw, ad)  # more slots than the library holds


def test_abi_rejects_bad_input():
    """The entry points' own checks, below the Python ones."""
    from mhppo import _lib
    from mhppo.policy import Policy
    ac, aw, ad = nets(17)
    pol = Policy("coop", 2, 1, 2, ac, aw, ad)
    L = _lib.lib()
    obs = torch.zeros((4, pol.obs_dim), device="cuda")
    a_d = torch.zeros((4, 2, 1), dtype=torch.int32, device="cuda")
    out = torch.zeros((4, 4), dtype=torch.float64, device="cuda")
    dc, _ = ac.mlp_desc()
    dw, _ = aw.mlp_desc()
    dd, _ = ad.mlp_desc()
    st = _lib.stream_ptr()

    def cfg_with(**kw):
        c = _lib.EnvCfg.from_buffer_copy(pol.cfg)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    big_p, bad_v = cfg_with(nb_ped=33), cfg_with(variant=9)
    assert L.mhppo_policy_act(ctypes.byref(big_p), ctypes.byref(dc), ctypes.byref(dw), _lib.ptr(obs), _lib.ptr(a_d), 4,
                              _lib.ptr(out), st) == -1
    assert b"nb_ped" in L.mhppo_last_error()
    dims = (ctypes.c_int32 * 4)()
    assert L.mhppo_policy_dims(ctypes.byref(bad_v), dims) == -1
    # a critic / the choice actor where a continuous actor belongs; a continuous actor as the choice actor
    assert L.mhppo_policy_act(ctypes.byref(pol.cfg), ctypes.byref(dd), ctypes.byref(dw), _lib.ptr(obs), _lib.ptr(a_d),
                              4, _lib.ptr(out), st) == -1
    assert L.mhppo_policy_decide(ctypes.byref(pol.cfg), ctypes.byref(dc), _lib.ptr(obs), 4, _lib.ptr(a_d), None,
                                 st) == -1
    assert L.mhppo_policy_decide(ctypes.byref(pol.cfg), ctypes.byref(dd), None, 4, _lib.ptr(a_d), None, st) == -1
    torch.cuda.synchronize()
    assert not out.any() and not a_d.any()
