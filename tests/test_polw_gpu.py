"""The wide device-resident MlpPolicy (csrc/xarm_k_acw.hip) through DevicePolicy's "wide" backend on the GPU: rows against the host
build's bits and against float64, rows independent of their batch, fresh noise per replay of a captured call, the in-kernel
normalisation, predict on twin envs, and the act call's logp / value against what the wide PPO update computes at call start."""
import types

import numpy as np
import pytest
import torch

import policy_host as PH
import ppow_host as W

pytestmark = pytest.mark.gpu
SIZES = (1, 31, 33, 65, 200)
SHAPES = (W.SHAPE_A, W.SHAPE_REF, W.SHAPE_ODD, W.SHAPE_MAX, W.SHAPE_CROSS)
KEYS = ("action", "env_action", "logp", "value")


def policy_of(shape, **kw):
    from gym_xarm_amd.device_policy import DevicePolicy
    model = W.model_of(shape).cuda()
    pol = DevicePolicy(model, wide=True if shape == W.SHAPE_CROSS else None, **kw)
    assert pol.backend == "wide"
    return model, pol


def rows_of(shape, E, seed=0):
    return np.random.RandomState(40 + seed + shape[0]).uniform(-2.5, 2.5, (E, shape[0])).astype(np.float32)


def act(pol, obs, E, **kw):
    out = pol.alloc_out(E)
    for v in out.values():
        v.fill_(float("nan"))
    return {k: v.cpu().numpy() for k, v in pol.act_into(out, obs, **kw).items()}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d-A%d-%dx%d-%s" % s)
def test_rows_equal_the_host_build_and_do_not_depend_on_the_batch(shape):
    model, pol = policy_of(shape, seed=5, row_offset=3)
    w = W.weights_of(model)
    full = rows_of(shape, 200)
    host = W.host_act(w, full, shape, seed=5, row_offset=3)
    m64 = W.model_of(shape).double()
    with torch.no_grad():
        mean64, v64 = m64.pi(torch.from_numpy(full).double()).numpy(), m64.value(torch.from_numpy(full).double()).numpy()
    for E in SIZES:
        pol.calls.zero_()
        dev = act(pol, torch.from_numpy(full[:E]).cuda(), E)
        for k in KEYS:
            assert PH.bits(dev[k]) == PH.bits(host[k][:E]), (E, k)          # the host build's bits, and the rows of the 200-row batch
        det = act(pol, torch.from_numpy(full[:E]).cuda(), E, deterministic=True)
        # float32 chains of at most 256 terms per layer against float64
        assert np.abs(det["action"] - mean64[:E]).max() <= 1e-4 * max(1.0, np.abs(mean64).max()) and np.abs(det["value"] - v64[:E]).max() <= 1e-4 * max(1.0, np.abs(v64).max())
        assert np.array_equal(det["env_action"], np.clip(det["action"], -1.0, 1.0))
    assert int(pol.calls) == 1


def test_only_the_requested_outputs_are_written_and_the_value_tower_can_be_skipped():
    shape, E = W.SHAPE_A, 33
    model, pol = policy_of(shape, seed=1)
    obs = torch.from_numpy(rows_of(shape, E)).cuda()
    ref = act(pol, obs, E, deterministic=True)
    out = {"env_action": torch.full((E, shape[1]), float("nan"), device="cuda")}
    pol.act_into(out, obs, deterministic=True)
    assert np.array_equal(out["env_action"].cpu().numpy(), ref["env_action"])


def test_normalisation_in_the_call_equals_the_call_on_normalised_rows():
    shape, E = (30, 4, 256, 3, "relu"), 65
    od, gd = 24, 3
    model, pol = policy_of(shape, seed=2)
    rs = np.random.RandomState(3)
    raw = rs.uniform(-3.0, 3.0, (E, shape[0])).astype(np.float32)
    stats = np.concatenate([rs.uniform(-0.5, 0.5, shape[0]), rs.uniform(0.5, 2.0, shape[0]), np.zeros(4)])
    venv = types.SimpleNamespace(stats=torch.from_numpy(stats).cuda(), dim=shape[0], clip_obs=10.0, eps=1e-8)
    obs = {k: torch.from_numpy(p).cuda() for k, p in zip(("observation", "achieved_goal", "desired_goal"), PH.split(raw, od, gd))}
    fused = act(pol, obs, E, normalize=venv)
    host = W.host_act(W.weights_of(model), raw, shape, goal_dim=gd, stats=stats, seed=2)
    normed = host["workspace"][:E * shape[0]].reshape(E, shape[0]).copy()           # the prep launch's rows
    expect = np.clip((raw.astype(np.float64) - stats[:shape[0]]) / np.sqrt(stats[shape[0]:2 * shape[0]] + 1e-8), -10.0, 10.0).astype(np.float32)
    assert np.array_equal(normed, expect)
    pol.calls.zero_()
    plain = act(pol, torch.from_numpy(normed).cuda(), E)
    for k in KEYS:
        assert PH.bits(fused[k]) == PH.bits(host[k]) and PH.bits(fused[k]) == PH.bits(plain[k]), k


def test_captured_act_into_draws_fresh_noise_per_replay():
    shape, E = W.SHAPE_REF, 200
    model, cap = policy_of(shape, seed=21, act_rows=E)
    _, twin = policy_of(shape, seed=21, act_rows=E)
    twin.model = model
    obs = torch.from_numpy(rows_of(shape, E)).cuda()
    out, ref = cap.alloc_out(E), twin.alloc_out(E)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.act_into(out, obs)                               # warm-up call
    torch.cuda.current_stream().wait_stream(side)
    twin.act_into(ref, obs)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.act_into(out, obs)
    seen = []
    for k in range(3):
        graph.replay()
        twin.act_into(ref, obs)
        torch.cuda.synchronize()
        for key in KEYS:
            assert torch.equal(out[key], ref[key]), (k, key)
        assert int(cap.calls) == int(twin.calls) == k + 2
        seen.append(out["action"].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    host = W.host_act(W.weights_of(model), rows_of(shape, E), shape, seed=21, calls=np.array([3], np.int64))
    assert PH.bits(seen[2].cpu().numpy()) == PH.bits(host["action"])


def test_predict_with_a_frozen_normaliser_on_twin_envs():
    import gym_xarm_amd
    from gym_xarm_amd import train as TR
    from gym_xarm_amd.device_policy import DevicePolicy
    from gym_xarm_amd.normalize import DeviceVecNormalize
    envs = [gym_xarm_amd.make("XarmReach-v0", num_envs=64, seed=11) for _ in range(2)]
    venvs = []
    for env in envs:
        venv = DeviceVecNormalize(env, monitor_capacity=1024)
        venv.reset()
        g = torch.Generator(device="cuda")
        g.manual_seed(2)
        for _ in range(6):
            venv.step(torch.rand(env.num_envs, env.act_dim, device="cuda", generator=g) * 2 - 1)
        venv.training = False
        venvs.append(venv)
    torch.manual_seed(4)
    model = TR.ActorCritic(venvs[0].dim, envs[0].act_dim, (128, 128), "relu").cuda()
    pa, pb = DevicePolicy(model), DevicePolicy(model)
    assert pa.backend == "wide"
    oa, ob = envs[0].reset(), envs[1].reset()
    for k in range(8):
        aa, ab = pa.predict(oa, normalize=venvs[0]), pb.predict(ob, normalize=venvs[1])
        assert torch.equal(aa, ab) and bool(torch.isfinite(aa).all()) and float(aa.abs().max()) <= 1.0, k
        oa, ob = envs[0].step(aa)[0], envs[1].step(ab)[0]
    assert int(pa.calls) == 0
    for env in envs:
        env.close()


def test_logp_and_value_are_the_update_s_call_start_rows():
    """a deterministic act call's action is the mean: stored as the rollout's action, the wide PPO update's call-start forward gives the
    same value and the same log-probability for every row, bit for bit (the workspace's value and old_logp parts)"""
    from gym_xarm_amd.device_ppo import DevicePPO
    shape, T, E = W.SHAPE_REF, 2, 33
    model, pol = policy_of(shape)
    ppo = DevicePPO(model, E, n_steps=T, n_epochs=1, batch_size=40, lr=0.0)
    obs = torch.from_numpy(rows_of(shape, T * E)).cuda()
    out = pol.act(obs, deterministic=True)
    ppo.buffers["obs"].copy_(obs.view(T, E, -1))
    ppo.buffers["action"].copy_(out["action"].view(T, E, -1))
    ppo.update(obs[:E].contiguous(), shuffle=False)
    work, o = ppo.buffers["workspace"], W.geometry(T, E, shape, 1, 40)["work"]
    assert torch.equal(work[o["value"]:o["value"] + T * E], out["value"]) and torch.equal(work[o["old_logp"]:o["old_logp"] + T * E], out["logp"])
    assert torch.equal(work[o["value"] + T * E:o["value"] + T * E + E], out["value"][:E])       # last_obs's rows are the first E
