"""The device shuffle (csrc/xarm_k_rollout.hip) on the GPU: xarm_perm_fill bit for bit the host build's (tests/rollout_host.py), eager
and replayed from a captured graph, the shuffle inside DevicePPO.update against a twin fed the host build's permutation on both
backends, and train(shuffle="device")."""
import copy

import numpy as np
import pytest
import torch

import a2c_host as AH
import rollout_host as RH

pytestmark = pytest.mark.gpu
GPU_PERM_SIZES = tuple(n for n in RH.PERM_SIZES if n <= 4097) + (4097,)


def device_fill(perm, calls, seed):
    from gym_xarm_amd import _native
    import ctypes as C
    L = _native.load()
    rc = L.xarm_perm_fill(C.c_void_p(perm.data_ptr()), perm.shape[0], perm.shape[1], seed, C.c_void_p(calls.data_ptr()),
                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.xarm_last_error(None)


@pytest.mark.parametrize("N", GPU_PERM_SIZES)
def test_perm_fill_is_the_host_build(N):
    start = (1 << 32) - 1                          # the second call's counter has a high word
    perm = torch.full((3, N), -1, dtype=torch.int32, device="cuda")
    calls = torch.tensor([start], dtype=torch.int64, device="cuda")
    for c in (start, start + 1):
        device_fill(perm, calls, 11)
        assert int(calls[0]) == c + 1
        assert RH.bits(perm.cpu().numpy()) == RH.bits(RH.perm_fill(3, N, 11, c)[0]), (N, c)


def test_a_captured_fill_draws_a_fresh_shuffle_per_replay():
    N, c0 = 1000, 5
    perm = torch.zeros(2, N, dtype=torch.int32, device="cuda")
    calls = torch.tensor([c0 - 1], dtype=torch.int64, device="cuda")
    device_fill(perm, calls, 3)                    # the kernels are loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        device_fill(perm, calls, 3)
    assert int(calls[0]) == c0                     # a capture executes nothing
    for c in (c0, c0 + 1, c0 + 2):
        graph.replay()
        assert RH.bits(perm.cpu().numpy()) == RH.bits(RH.perm_fill(2, N, 3, c)[0]), c
    assert int(calls[0]) == c0 + 3


def ppo_pair(D, A, T, E, B, wide):
    from gym_xarm_amd.device_ppo import DevicePPO
    from gym_xarm_amd.train import ActorCritic
    if wide:
        torch.manual_seed(5)
        model = ActorCritic(D, A, (64, 64), "tanh")
    else:
        model = AH.model_of(D, A, 1.0)
    out = []
    for shuffle in ("device", "torch"):
        m = copy.deepcopy(model).cuda()
        out.append(DevicePPO(m, E, n_steps=T, n_epochs=2, batch_size=B, seed=9, wide=True if wide else None, shuffle=shuffle, target_kl=0.5))
    return out


@pytest.mark.parametrize("wide", (False, True))
@pytest.mark.parametrize("E,B", ((13, 20), (200, 300)))
def test_update_with_the_device_shuffle_is_the_twin_fed_the_host_permutation(E, B, wide):
    D, A, T = 14, 4, 5
    dev, twin = ppo_pair(D, A, T, E, B, wide)
    assert dev.backend == twin.backend == ("wide" if wide else "tile64") and twin.perm_calls is None
    b = AH.make_batch(D, A, T, E, 1.0)
    last = torch.from_numpy(b["last_obs"]).cuda()
    for round_ in range(2):                        # the second update draws at calls = 1
        for p in (dev, twin):
            for k in ("obs", "action", "reward", "done", "use"):
                p.buffers[k].copy_(torch.from_numpy(b[k]))
        dev.update(last)
        twin.perm.copy_(torch.from_numpy(RH.perm_fill(2, T * E, 9, round_)[0]))
        twin.update(last, shuffle=False)
        assert int(dev.perm_calls[0]) == round_ + 1 and torch.equal(dev.perm, twin.perm)
        assert int(dev.step[0]) == int(twin.step[0]) > 0
        for x, y in zip(list(dev.params()) + dev.exp_avg + dev.exp_avg_sq + [dev.stats], list(twin.params()) + twin.exp_avg + twin.exp_avg_sq + [twin.stats]):
            assert RH.bits(x.detach().cpu().numpy()) == RH.bits(y.detach().cpu().numpy())
    dev.update(last, shuffle=False)                # shuffle=False still skips the fill
    assert int(dev.perm_calls[0]) == 2


def test_train_with_the_device_shuffle():
    """train(algo="ppo", device_update=True, shuffle="device"): a smoke run - one fill per update, finite parameters - on both backends"""
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    for kw in (dict(), dict(net_arch=(64, 64), activation="relu")):
        env = gym_xarm_amd.make("XarmReach-v0", num_envs=256, seed=0)
        model, venv, hist = train(env=env, updates=4, algo="ppo", device_update=True, device_policy=True, device_normalize=True, quiet=True, log_every=2,
                                  n_steps=4, n_epochs=2, batch_size=256, shuffle="device", **kw)
        assert len(hist) == 2 and all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_the_device_shuffle_needs_the_device_update():
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=64, seed=0)
    with pytest.raises(ValueError, match="DevicePPO"):
        train(env=env, updates=2, quiet=True, algo="ppo", shuffle="device")
    env.close()
