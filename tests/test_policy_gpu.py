"""The device-resident MlpPolicy on the MI355X (gym_xarm_amd/device_policy.py DevicePolicy, csrc/xarm_k_policy.hip): the kernel
against the host build of the same core bit for bit at the tile and workgroup edges, one large batch, determinism, independence
of the batch, weights read in place, the frozen normaliser fused into the call, `predict` on a live env, a captured act_into
against eager calls, and the training driver with the device policy."""
import copy
import types

import numpy as np
import pytest
import torch

import policy_host as PH
from gym_xarm_amd.device_policy import DevicePolicy

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 64, 65, 1000)
KEYS = ("action", "env_action", "logp", "value")


def to_dev(rows, od, gd):
    t = [None if p is None else torch.from_numpy(p).cuda() for p in PH.split(rows, od, gd)]
    return t[0] if t[1] is None else {"observation": t[0], "achieved_goal": t[1], "desired_goal": t[2]}


def frozen(stats, D):
    """what act_into reads of a DeviceVecNormalize: the statistics tensor and the settings"""
    return types.SimpleNamespace(stats=torch.from_numpy(stats).cuda(), dim=D, clip_obs=10.0, eps=1e-8)


def device_act(pol, obs, E, deterministic=False, normalize=None, keys=KEYS):
    """one act_into on outputs filled with NaN"""
    out = {k: v for k, v in pol.alloc_out(E).items() if k in keys}
    for v in out.values():
        v.fill_(float("nan"))
    pol.act_into(out, obs, deterministic, normalize)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same(dev, host, what):
    for k, v in dev.items():
        assert PH.bits(v) == PH.bits(host[k]), (what, k, float(np.nanmax(np.abs(v.astype(np.float64) - host[k]))))


@pytest.mark.parametrize("A", PH.ACT_DIMS)
@pytest.mark.parametrize("od,gd", PH.WIDTHS)
def test_kernel_equals_the_host_build_bit_for_bit(od, gd, A):
    """every batch size x (stochastic, stochastic on frozen statistics, deterministic, stochastic with null logp / value on frozen
    statistics) x three consecutive calls, all four outputs, NaN-filled before each call; the weights x 4 set at act_dim 8"""
    c = PH.case(od, gd, A, 4.0 if A == 8 else 1.0)
    D = c["D"]
    model = copy.deepcopy(c["model"]).cuda()
    rng = np.random.RandomState(D + A)
    stats = np.concatenate([rng.uniform(-1, 1, D), rng.uniform(0.05, 4, D), [0.0, 1.0, 1000.0, 1000.0]])
    modes = ((False, False, KEYS), (False, True, KEYS), (True, False, KEYS), (False, True, KEYS[:2]))
    for E in SIZES:
        rows = c["rows"][:E]
        obs = to_dev(rows, od, gd)
        for m, (det, with_stats, keys) in enumerate(modes):
            if E == 1000 and m in (1, 2):
                continue
            pol = DevicePolicy(model, seed=100 + m, row_offset=5 * E)
            calls = np.zeros(1, np.int64)
            for k in range(3):
                dev = device_act(pol, obs, E, det, frozen(stats, D) if with_stats else None, keys)
                host = PH.host_act(c["w"], rows, od, gd, stats=stats if with_stats else None, deterministic=det, seed=100 + m,
                                   row_offset=5 * E, calls=calls, logp="logp" in keys, value="value" in keys)
                assert_same(dev, host, (E, m, k))
                assert int(pol.calls) == calls[0] == (0 if det else k + 1)


def test_one_large_batch_equals_the_host_build():
    od, gd, A, E = 8, 3, 4, 65536
    c = PH.case(od, gd, A, 1.0)
    rows = np.random.RandomState(8).uniform(-10, 10, (E, c["D"])).astype(np.float32)
    pol = DevicePolicy(copy.deepcopy(c["model"]).cuda(), seed=12, row_offset=(1 << 32) - 1000)      # global rows cross 2^32
    dev = device_act(pol, to_dev(rows, od, gd), E)
    assert_same(dev, PH.host_act(c["w"], rows, od, gd, seed=12, row_offset=(1 << 32) - 1000), "65536")


def test_same_inputs_twice_give_the_same_bits_and_a_row_does_not_depend_on_its_batch():
    od, gd, A = 24, 3, 4
    c = PH.case(od, gd, A, 1.0)
    model = copy.deepcopy(c["model"]).cuda()
    obs = to_dev(c["rows"], od, gd)
    a, b = (device_act(DevicePolicy(model, seed=3), obs, 1000) for _ in range(2))
    assert_same(a, b, "run to run")
    one = device_act(DevicePolicy(model, seed=3, row_offset=7), to_dev(c["rows"][7:8], od, gd), 1)
    assert_same(one, {k: v[7:8] for k, v in a.items()}, "row 7 of 1000 against a batch of one")
    other = device_act(DevicePolicy(model, seed=4), obs, 1000)
    assert not (other["action"] == a["action"]).any() and PH.bits(other["value"]) == PH.bits(a["value"])


def test_weights_are_read_in_place():
    od, gd, A = 8, 3, 4
    c = PH.case(od, gd, A, 1.0)
    model = copy.deepcopy(c["model"]).cuda()
    pol = DevicePolicy(model)
    obs = to_dev(c["rows"][:65], od, gd)
    before = device_act(pol, obs, 65, deterministic=True)
    with torch.no_grad():
        model.pi[4].weight.mul_(2.0)                         # in place: same storage, no repacking
    after = device_act(pol, obs, 65, deterministic=True)
    assert not (after["action"] == before["action"]).all() and PH.bits(after["value"]) == PH.bits(before["value"])
    assert_same(after, PH.host_act(PH.weights_of(model), c["rows"][:65], od, gd, deterministic=True), "the new weights")


def _warm_normaliser(env, steps=12):
    from gym_xarm_amd.normalize import DeviceVecNormalize
    venv = DeviceVecNormalize(env, monitor_capacity=1024)
    venv.reset()
    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    for _ in range(steps):
        venv.step(torch.rand(env.num_envs, env.act_dim, device="cuda", generator=g) * 2 - 1)
    venv.training = False
    return venv


def test_frozen_normaliser_in_the_call_equals_act_on_the_wrappers_output():
    import gym_xarm_amd
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=64, seed=6)
    venv = _warm_normaliser(env)
    stats = venv.stats.clone()
    model = PH.make_model(venv.dim, env.act_dim).cuda()
    fused, plain = DevicePolicy(model, seed=9), DevicePolicy(model, seed=9)
    obs, rew, done, info = env.step(torch.zeros(64, env.act_dim, device="cuda"))
    nobs = venv.step_into(venv.alloc_out(), obs, rew, done)["nobs"]
    assert torch.equal(venv.stats, stats)                     # frozen
    for k in range(2):
        a, b = device_act(fused, obs, 64, normalize=venv), device_act(plain, nobs, 64)
        assert_same(a, b, k)
    env.close()


def test_predict_on_a_live_env_gives_finite_and_repeatable_trajectories():
    import gym_xarm_amd
    ea, eb = (gym_xarm_amd.make("XarmReach-v0", num_envs=64, seed=11) for _ in range(2))
    va = _warm_normaliser(ea)
    vb = _warm_normaliser(eb)
    assert torch.equal(va.stats, vb.stats) and torch.equal(ea.get_state(), eb.get_state())
    model = PH.make_model(va.dim, ea.act_dim).cuda()
    pa, pb = DevicePolicy(model), DevicePolicy(model)
    oa, ob = ea.reset(), eb.reset()
    moved = 0
    for k in range(25):
        aa, ab = pa.predict(oa, normalize=va), pb.predict(ob, normalize=vb)
        assert torch.equal(aa, ab) and bool(torch.isfinite(aa).all()) and float(aa.abs().max()) <= 1.0, k
        moved += int((aa != 0).any())
        oa, _, _, _ = ea.step(aa)
        ob, _, _, _ = eb.step(ab)
        for key in oa:
            assert torch.equal(oa[key], ob[key]) and bool(torch.isfinite(oa[key]).all()), (k, key)
    assert moved == 25 and int(pa.calls) == 0                 # deterministic calls do not tick
    ea.close()
    eb.close()


def test_captured_act_into_replays_like_eager_calls():
    """default queue settings, the test's own process: four replays draw fresh noise and each equals its eager call on a twin"""
    od, gd, A, E = 24, 3, 4, 1000
    c = PH.case(od, gd, A, 1.0)
    model = copy.deepcopy(c["model"]).cuda()
    cap, twin = DevicePolicy(model, seed=21), DevicePolicy(model, seed=21)
    obs = to_dev(c["rows"], od, gd)
    out, ref = cap.alloc_out(E), twin.alloc_out(E)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.act_into(out, obs)                               # warm-up call
    torch.cuda.current_stream().wait_stream(side)
    twin.act_into(ref, obs)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.act_into(out, obs)                               # no allocation, no host read: it captures (nothing runs yet)
    torch.cuda.synchronize()
    assert int(cap.calls) == 1
    seen = []
    for k in range(4):
        for key, part in zip(("observation", "achieved_goal", "desired_goal"), PH.split(np.roll(c["rows"], k + 1, 0), od, gd)):
            obs[key].copy_(torch.from_numpy(part))           # the static inputs, rewritten in place
        graph.replay()
        twin.act_into(ref, obs)
        torch.cuda.synchronize()
        for key in KEYS:
            assert torch.equal(out[key], ref[key]), (k, key)
        assert int(cap.calls) == int(twin.calls) == k + 2
        seen.append(out["action"].cpu().numpy())
    host = PH.host_act(c["w"], np.roll(c["rows"], 4, 0), od, gd, seed=21, calls=np.array([4], np.int64))
    assert PH.bits(seen[3]) == PH.bits(host["action"])
    for i in range(4):
        for j in range(i):
            assert not (seen[i] == seen[j]).any()


@pytest.mark.parametrize("device_normalize", (False, True))
def test_driver_with_the_device_policy(device_normalize):
    """a smoke run, not a learning curve"""
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=256, seed=0)
    model, venv, hist = train(env=env, updates=20, device_policy=True, device_normalize=device_normalize, quiet=True, log_every=10)
    assert len(hist) == 2
    for rec in hist:
        assert all(np.isfinite(v) for v in rec.values()), rec
    assert hist[-1]["env_steps"] == 20 * 5 * 256 and venv.monitor.n == 20 * 5 * 256 // 25
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
