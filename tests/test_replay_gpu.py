"""The device-resident uniform replay buffer on the MI355X (gym_xarm_amd/replay.py DeviceReplayBuffer, csrc/xarm_k_replay.hip): ring and
samples against the host build of the same core bit for bit, a captured sample, the learners' update_from against a twin fed through
update(), and the drivers on the flat Handover env and on dense Reach."""
import copy
import ctypes as C
import math

import numpy as np
import pytest
import torch

import replay_host as RH
from gym_xarm_amd.replay import DeviceReplayBuffer

pytestmark = pytest.mark.gpu
FIELDS = ("obs", "next_obs", "action", "reward", "done", "use", "env", "time")


def make_env(kind, E):
    if kind == "flat":
        return RH.FlatScripted(RH.ep_lens(E), obs_dim=29, act_dim=8, device="cuda")                    # Handover NoGoal's record
    return RH.GoalScripted(RH.ep_lens(E), obs_dim=25, goal_dim=3, act_dim=4, device="cuda")            # PickAndPlace's triple


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


def make_stats(D, seed=3):
    rng = np.random.default_rng(seed)
    s = np.zeros(2 * D + 4)
    s[:D] = rng.normal(0.0, 50.0, D)
    s[D:2 * D] = rng.uniform(0.5, 4e5, D)
    s[D + 1], s[D + 2] = 0.0, 1e-3      # a zero variance and one that clips
    return s


class Norm:
    """what sample_into reads of a DeviceVecNormalize"""

    def __init__(self, stats, clip_obs=10.0, eps=1e-8):
        self.stats, self.dim, self.clip_obs, self.eps = torch.from_numpy(stats).cuda(), (len(stats) - 4) // 2, clip_obs, eps


def pair(kind, E, T, steps, seed=0):
    env = make_env(kind, E)
    host = RH.HostReplay(E, T, env.obs_dim, env.goal_dim, env.act_dim, seed=seed)
    buf = DeviceReplayBuffer(env, buffer_size=T * E, seed=seed)
    assert buf.horizon == T and buf.record_floats == host.R and buf.dim == host.D
    RH.collect(env, [host, buf], steps)
    return env, host, buf


def same(out, ref, what):
    torch.cuda.synchronize()
    for k in FIELDS:
        assert bits(out[k]) == bits(ref[k]), (what, k)


@pytest.mark.parametrize("kind", ["flat", "goal"])
@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("E", [1, 3, 65])
def test_add_and_sample_equal_the_host_build(kind, E, T):
    stats = None
    for steps in (T - 1, 2 * T + 1):                      # before and after the ring wraps
        env, host, buf = pair(kind, E, T, steps)
        assert bits(buf.ring) == bits(host.ring) and buf.clock.tolist() == host.clock.tolist() == [steps, 0]
        stats = make_stats(host.D)
        for B in (1, 63, 64, 65, 257):
            for st in (None, stats):
                out = buf.sample(B, None if st is None else Norm(st))
                same(out, host.sample(B, stats=st), (steps, B, st is not None))
        assert buf.clock.tolist() == host.clock.tolist() == [steps, 10]
    # two calls across a sample_calls of 2^32 - 1 (the buffers of the wrapped case)
    host.clock[1] = 2 ** 32 - 1
    buf.clock[1] = 2 ** 32 - 1
    a, b = buf.sample(65, Norm(stats)), buf.sample(65)
    same(a, host.sample(65, stats=stats), "2^32 - 1")
    same(b, host.sample(65), "2^32")
    assert buf.clock.tolist() == [2 * T + 1, 2 ** 32 + 1] and not torch.equal(a["time"] * E + a["env"], b["time"] * E + b["env"])


def test_empty_buffer_and_the_handling_switch():
    env = make_env("flat", 3)
    buf = DeviceReplayBuffer(env, buffer_size=3 * 12)
    out = {k: torch.full_like(v, 77) for k, v in buf.alloc_out(70).items()}
    buf.sample_into(out)
    torch.cuda.synchronize()
    for k in FIELDS:
        assert not bool(out[k].any()), k
    host = RH.HostReplay(3, 12, 29, 0, 8)
    buf.clock[1] = 0
    RH.collect(env, [host, buf], 12)
    buf.handle_timeout_termination = False
    off = buf.sample(300)
    same(off, host.sample(300, handle_timeout=False), "handling off")
    buf.handle_timeout_termination = True
    on = buf.sample(300)
    same(on, host.sample(300, handle_timeout=True), "handling on")
    ends = lambda o: torch.tensor([(int(t) + 1) % RH.ep_lens(3)[int(e)] == 0 for e, t in zip(o["env"].cpu(), o["time"].cpu())])
    assert torch.equal(off["done"].cpu() != 0, ends(off)) and torch.equal(on["done"].cpu() != 0, ends(on) & (on["env"].cpu() % 2 == 1))
    assert bool(ends(on).any()) and bool((on["done"] != 0).any())


def test_errors_are_reported_and_nothing_is_launched():
    from gym_xarm_amd import _native
    L = _native.load()
    lay = _native.XarmReplayLayout(4, 8, 29, 0, 8)
    assert L.xarm_replay_record_floats(C.byref(lay)) == 2 * 29 + 8 + 3
    assert L.xarm_replay_record_floats(None) == -1 and b"layout is NULL" in L.xarm_last_error(None)
    assert L.xarm_replay_record_floats(C.byref(_native.XarmReplayLayout(4, 0, 29, 0, 8))) == -1 and b"horizon" in L.xarm_last_error(None)
    assert L.xarm_replay_add(C.byref(lay), *([None] * 12)) == -1 and b"NULL pointer" in L.xarm_last_error(None)
    assert L.xarm_replay_sample(C.byref(lay), None, None, 0, 16, 1, None, 10.0, 1e-8, *([None] * 9)) == -1 and b"NULL pointer" in L.xarm_last_error(None)
    assert L.xarm_replay_sample(C.byref(lay), None, None, 0, -1, 1, None, 10.0, 1e-8, *([None] * 9)) == -1 and b"batch" in L.xarm_last_error(None)
    assert L.xarm_replay_sample(C.byref(lay), None, None, 0, 0, 1, None, 10.0, 1e-8, *([None] * 9)) == 0          # batch 0: nothing to do
    assert L.xarm_replay_add(C.byref(_native.XarmReplayLayout(0, 8, 29, 0, 8)), *([None] * 12)) == 0              # no envs
    env, host, buf = pair("flat", 3, 4, 2)
    with pytest.raises(ValueError, match="observation width"):
        buf.sample(8, Norm(make_stats(30)))
    st = torch.zeros(1, dtype=torch.float64, device="cuda")
    out = buf.alloc_out(8)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = [p(out[k]) for k in FIELDS]
    assert L.xarm_replay_sample(C.byref(buf.layout), p(buf.ring), p(buf.clock), 0, 8, 1, p(st), 0.0, 1e-8, *args, None) == -1
    assert b"clip_obs" in L.xarm_last_error(None)
    assert L.xarm_replay_sample(C.byref(buf.layout), p(buf.ring), p(buf.clock), 0, 8, 1, p(st), 10.0, 0.0, *args, None) == -1
    assert b"eps" in L.xarm_last_error(None)
    torch.cuda.synchronize()
    assert buf.clock.tolist() == [2, 0]


def test_three_replays_of_a_captured_sample_are_three_fresh_batches():
    env, host, buf = pair("goal", 65, 5, 11)
    norm = Norm(make_stats(host.D))
    out = buf.alloc_out(257)
    buf.sample_into(out, norm)                            # a warm-up call; the clock is put back after it
    buf.clock[1] = 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        buf.sample_into(out, norm)
    got = []
    for _ in range(3):
        graph.replay()
        got.append({k: v.clone() for k, v in out.items()})
    torch.cuda.synchronize()
    assert buf.clock.tolist() == [11, 3]
    for k, g in enumerate(got):
        same(g, host.sample(257, stats=norm.stats.cpu().numpy()), "replay %d" % k)
    assert not torch.equal(got[0]["time"], got[1]["time"]) and not torch.equal(got[1]["time"], got[2]["time"])


def state_of(d):
    return [p.detach().clone() for p in d.params()] + [t.clone() for t in d.exp_avg + d.exp_avg_sq] + [d.step.clone(), d.stats.clone()]


def learner(algo, D, A, arch, activation, B):
    from gym_xarm_amd.device_sac import DeviceSAC
    from gym_xarm_amd.device_td3 import DeviceTD3
    from gym_xarm_amd.sac import SacPolicy
    from gym_xarm_amd.td3 import Td3Policy
    g = torch.random.get_rng_state()
    torch.manual_seed(11)
    model = (SacPolicy if algo == "sac" else Td3Policy)(D, A, arch, activation)
    torch.random.set_rng_state(g)
    out = []
    for _ in range(2):
        m = copy.deepcopy(model).cuda()
        out.append(DeviceSAC(m, B, seed=5) if algo == "sac" else DeviceTD3(m, B, seed=5, policy_delay=2))
    return out


@pytest.mark.parametrize("kind", ["flat", "goal"])
@pytest.mark.parametrize("arch", [((64, 64), "tanh"), ((256, 256, 256), "relu")], ids=["64-64-tanh", "256x3-relu"])
@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_update_from_the_buffer_equals_update_on_a_twin(algo, arch, kind):
    """update_from(buffer, venv) - the sample kernel writing the learner's own batch tensors, normalised inside - against a twin model fed
    update(batch), its batch sampled without stats from a twin buffer at the same clock and normalised by venv.normalize_rows"""
    from gym_xarm_amd.normalize import DeviceVecNormalize
    B, E, T = 96, 7, 6
    env, host, buf = pair(kind, E, T, 9, seed=2)
    env2, host2, buf2 = pair(kind, E, T, 9, seed=2)
    venv = DeviceVecNormalize(env, monitor_capacity=64)
    venv.stats.copy_(torch.from_numpy(make_stats(host.D)))
    one, two = learner(algo, host.D, env.act_dim, arch[0], arch[1], B)
    o, g = env.obs_dim, env.goal_dim
    for step in range(2):
        one.update_from(buf, venv)
        s = buf2.sample(B)
        nobs, nnext = torch.empty(B, host.D, device="cuda"), torch.empty(B, host.D, device="cuda")
        for dst, x in ((nobs, s["obs"]), (nnext, s["next_obs"])):
            parts = [x] if g == 0 else [x[:, :o].contiguous(), x[:, o:o + g].contiguous(), x[:, o + g:].contiguous()]
            venv.normalize_rows(dst, *parts)
        two.update({"obs": nobs, "next_obs": nnext, "action": s["action"], "reward": s["reward"], "done": s["done"], "use": s["use"]})
        torch.cuda.synchronize()
        assert bits(one.buffers["obs"]) == bits(nobs) and bits(one.buffers["next_obs"]) == bits(nnext)
        assert bits(one.buffers["done"]) == bits(s["done"]) and bits(one.buffers["use"]) == bits(s["use"])
    assert int(one.step[0]) == int(two.step[0]) == 2 and buf.clock.tolist() == buf2.clock.tolist() == [9, 2]
    for x, y in zip(state_of(one), state_of(two)):
        assert bits(x) == bits(y)
    assert bool(torch.isfinite(one.stats).all())
    with pytest.raises(ValueError, match="do not belong to this model"):
        learner(algo, host.D + 1, env.act_dim, arch[0], arch[1], B)[0].update_from(buf, venv)


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_drivers_run_on_the_flat_handover_env(algo):
    from gym_xarm_amd import sac, td3
    train, stats = (sac.train_sac, sac.STATS) if algo == "sac" else (td3.train_td3, td3.STATS)
    model, venv, hist = train("XarmPDHandoverNoGoal-v1", num_envs=64, steps=40, learning_starts=10, batch_size=64, device_update=True,
                              device_normalize=True, quiet=True)
    assert isinstance(venv.buffer, DeviceReplayBuffer) and venv.buffer.dim == 29 and venv.buffer.clock.tolist() == [40, 30]
    assert hist[-1]["updates"] == 30 and hist[-1]["n_use"] == 64.0
    assert all(math.isfinite(hist[-1][k]) for k in stats), hist[-1]
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_dense_reach_on_the_uniform_buffer_bootstraps_through_truncations():
    """XarmReach-v0's episodes are 25 steps and end only by the step limit: after 60 steps the ring holds truncations, every sampled done
    is 0 with the handling on and they show up as 1 with it off"""
    from gym_xarm_amd import sac
    model, venv, hist = sac.train_sac("XarmReach-v0", num_envs=64, steps=60, learning_starts=10, batch_size=64, device_update=True,
                                      device_normalize=True, quiet=True, replay="uniform", config={"reward_type": "dense", "GUI": False})
    buf = venv.buffer
    assert isinstance(buf, DeviceReplayBuffer) and buf.dim == venv.dim and hist[-1]["updates"] == 50
    assert all(math.isfinite(hist[-1][k]) for k in sac.STATS), hist[-1]
    R = buf.record_floats
    stored = buf.ring[:60]
    assert int(stored[..., R - 2].sum()) == int(stored[..., R - 1].sum()) == 2 * 64       # steps 25 and 50 of every env: done and timeout
    on = buf.sample(4096)
    buf.handle_timeout_termination = False
    off = buf.sample(4096)
    assert not bool(on["done"].any()) and bool(on["use"].all())
    assert bool(off["done"].any()) and torch.equal(off["done"] != 0, (off["time"] + 1) % 25 == 0)
