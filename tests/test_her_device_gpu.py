"""The device-resident HER buffer on the MI355X (gym_xarm_amd/her.py DeviceHerReplayBuffer, csrc/xarm_k_her.hip): the kernels
against the host build of the same core bit for bit, the device tables against the torch HerReplayBuffer after every add,
collect() + sample() on real envs, a captured sample_into against eager calls, and the envs left untouched by the buffer."""
import numpy as np
import pytest
import torch

import her_host as HH
from gym_xarm_amd.her import DeviceHerReplayBuffer, HerReplayBuffer, collect

pytestmark = pytest.mark.gpu

LAYOUTS = {"e6": (6, 4, 3, 2), "e70": (70, 55, 12, 8), "e129": (129, 8, 3, 4)}   # (E, obs, goal, act); e70: a 156-float record
BATCHES = (1, 63, 64, 65, 1000)
_states = {}


def device_buffer(E, o, g, a, **kw):
    label = HH.ScriptedEnv(HH.ep_lens(E), o, g, a, device="cuda")     # what the buffer is told: dims, device, reward
    return DeviceHerReplayBuffer(label, horizon=12, reward_fn=label.compute_reward, **kw)


def state40(name):
    """device and host buffers after the same 40 scripted steps (ring of 12 slots: wrapped three times); built once per layout"""
    if name not in _states:
        E, o, g, a = LAYOUTS[name]
        env = HH.ScriptedEnv(HH.ep_lens(E), o, g, a)
        dev, host = device_buffer(E, o, g, a, seed=11), HH.HostHer(E, 12, o, g, a, seed=11)
        collect(env, HH.Tee([dev, host]), env.policy, 40)
        assert dev.record_floats == host.R and dev.t == 40 == host.clock[0]
        _states[name] = (env, dev, host)
    return _states[name]


def bits(x):
    return np.ascontiguousarray(x).tobytes()


@pytest.mark.parametrize("strategy", ["future", "final", "episode"])
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_device_sample_equals_the_host_build_bit_for_bit(name, strategy):
    env, dev, host = state40(name)
    assert bits(dev.ring.cpu().numpy()) == bits(host.ring)
    for t in ("ep_end", "ep_first", "ep_start"):
        assert np.array_equal(getattr(dev, t).cpu().numpy(), getattr(host, t)), t
    dev.strategy, dev._strategy_id = strategy, HH.STRATEGY[strategy]
    for k, B in enumerate(BATCHES):
        dev.clock[1] = host.clock[1] = 100 + k
        fails = int(dev.fail_count.item()), int(host.fail_count[0])
        d, h = dev.sample(B), host.sample(B, strategy)
        n_her = h["n_her"]
        assert n_her == dev.n_her(B) == int(d["relabelled"].sum())
        for key, _, _ in HH.OUT:
            if key != "reward":
                assert bits(d[key].cpu().numpy()) == bits(h[key]), (key, B)
        assert bool(d["ok"].all())
        # the stored reward below the relabelled rows, the recomputed one on them
        assert bits(d["reward"][n_her:].cpu().numpy()) == bits(h["reward"][n_her:])
        expect = env.compute_reward(torch.from_numpy(h["next_achieved_goal"][:n_her]), torch.from_numpy(h["desired_goal"][:n_her]), None)
        assert torch.equal(d["reward"][:n_her].cpu(), expect)
        assert int(dev.clock[1].item()) == 101 + k == host.clock[1]
        assert (int(dev.fail_count.item()), int(host.fail_count[0])) == fails


def test_device_tables_equal_the_torch_buffer_after_every_add():
    E, o, g, a = LAYOUTS["e70"]
    env = HH.ScriptedEnv(HH.ep_lens(E), o, g, a)
    chk, dev = HerReplayBuffer(env, horizon=12), device_buffer(E, o, g, a)
    seen = []

    def compare(n):
        assert np.array_equal(dev.ep_end.cpu().numpy(), chk.ep_end.numpy()), n
        assert np.array_equal(dev.ep_start.cpu().numpy(), chk.ep_start.numpy()), n
        closed = chk.ep_end.numpy() >= 0
        L = np.asarray(HH.ep_lens(E))[None, :].repeat(12, 0)
        t = chk.slot_time.numpy()[:, None].repeat(E, 1)
        assert np.array_equal(dev.ep_first.cpu().numpy()[closed], ((t // L) * L)[closed]), n
        seen.append(dev.t)

    collect(env, HH.Tee([chk, dev], compare), env.policy, 40)
    assert seen == list(range(1, 41)) and dev.num_valid() == chk.num_valid()


def test_empty_device_buffer_raises_and_counts():
    dev = device_buffer(*LAYOUTS["e6"])
    out = dev.sample_into(dev.alloc_out(65))
    for k in dev.OUT_KEYS:
        assert not bool(out[k].any()), k
    assert int(dev.fail_count.item()) == 65
    with pytest.raises(RuntimeError, match="no finished episode"):
        dev.sample(4)


@pytest.mark.parametrize("env_id,E", [("XarmReach-v0", 512), ("XarmPDPickAndPlace-v0", 256)])
def test_collect_and_sample_on_a_real_env(env_id, E):
    import gym_xarm_amd
    env = gym_xarm_amd.make(env_id, num_envs=E, seed=3)
    buf = DeviceHerReplayBuffer(env, n_sampled_goal=4, seed=0)
    g = torch.Generator(device=env.device)
    g.manual_seed(0)
    collect(env, buf, lambda o: torch.rand(env.num_envs, env.act_dim, device=env.device, generator=g) * 2 - 1, 60)
    assert buf.t == 60 and buf.num_valid() >= 0.25 * 60 * E
    b = buf.sample(4096)
    rel = b["relabelled"]
    assert bool(b["ok"].all()) and int(rel.sum()) == round(0.8 * 4096) and bool(rel[:int(rel.sum())].all())
    d = torch.linalg.norm(b["next_achieved_goal"] - b["desired_goal"], dim=-1)
    expect = (d < 0.05).to(torch.float32)                           # xarm_reach.py:109-110, xarm_pick_and_place.py:163-165
    assert torch.equal(b["reward"][rel], expect[rel])
    print("relabelled mean reward %.4f, stored %.4f" % (float(b["reward"][rel].mean()), float(b["reward"][~rel].mean())))
    assert float(b["reward"][rel].mean()) > 5 * float(b["reward"][~rel].mean()) + 0.05
    s, e = b["time"] % buf.horizon, b["env"]
    end, first = buf.ep_end[s, e], buf.ep_first[s, e]
    assert bool((first <= b["time"]).all()) and bool((b["time"] <= b["goal_time"]).all()) and bool((b["goal_time"] <= end).all())
    assert bool((end < 60).all()) and bool((first >= 0).all())
    # the rows are the ring's records
    assert torch.equal(b["observation"], buf.ring[s, e, :env.obs_dim])
    sg = b["goal_time"] % buf.horizon
    o2 = 2 * env.obs_dim + env.goal_dim
    assert torch.equal(b["desired_goal"][rel], buf.ring[sg, e, o2:o2 + env.goal_dim][rel])
    assert b["observation"].device.type == "cuda" and b["observation"].shape == (4096, env.obs_dim)
    env.close()


def test_captured_sample_into_replays_like_eager_calls():
    import gym_xarm_amd
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=512, seed=3)
    cap, twin = DeviceHerReplayBuffer(env, seed=7), DeviceHerReplayBuffer(env, seed=7)
    g = torch.Generator(device=env.device)
    g.manual_seed(0)
    collect(env, HH.Tee([cap, twin]), lambda o: torch.rand(env.num_envs, env.act_dim, device=env.device, generator=g) * 2 - 1, 60)
    out, ref = cap.alloc_out(256), twin.alloc_out(256)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.sample_into(out)                                         # warm-up call: sample_calls 0
    torch.cuda.current_stream().wait_stream(side)
    twin.sample_into(ref)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap.sample_into(out)                                         # no allocation, no host read: it captures
    seen = []
    for k in range(3):
        graph.replay()
        twin.sample_into(ref)
        torch.cuda.synchronize()
        for key in cap.OUT_KEYS:
            assert torch.equal(out[key], ref[key]), (k, key)
        assert bool(out["ok"].all())
        seen.append((out["time"] * 512 + out["env"]).clone())
    assert int(cap.clock[1].item()) == 4 == int(twin.clock[1].item())   # the replays advanced the device clock
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2]) and not torch.equal(seen[0], seen[2])
    env.close()


def test_buffer_does_not_disturb_the_env():
    import gym_xarm_amd

    def run(with_buffer):
        env = gym_xarm_amd.make("XarmReach-v0", num_envs=512, seed=5)
        buf = DeviceHerReplayBuffer(env, seed=1) if with_buffer else None
        out = buf.alloc_out(1024) if with_buffer else None
        g = torch.Generator(device=env.device)
        g.manual_seed(2)
        obs, trace = env.reset(), []
        for _ in range(20):
            prev = {k: v.clone() for k, v in obs.items()}
            act = torch.rand(512, env.act_dim, device=env.device, generator=g) * 2 - 1
            obs, rew, done, info = env.step(act)
            if with_buffer:
                d = (done != 0)[:, None]
                term = info["terminal_observation"]
                nxt = {"observation": torch.where(d, term, obs["observation"]),
                       "achieved_goal": torch.where(d, env.achieved_goal_of(term), obs["achieved_goal"])}
                buf.add(prev, nxt, act, rew, done)
                buf.sample_into(out)
            trace.append([obs[k].clone() for k in sorted(obs)] + [rew.clone(), done.clone()])
        state = env.get_state().clone()
        env.close()
        return trace, state

    (a, sa), (b, sb) = run(True), run(False)
    assert torch.equal(sa, sb)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert torch.equal(u, v)


def test_offsets_past_two_to_the_31_floats():
    """a ring of 4096 x 4096 x 156 floats (2.6e9, 10.5 GB): add into the last slot and sample over all of them"""
    E, o, g, a, T = 4096, 55, 12, 8, 4096
    label = HH.ScriptedEnv(HH.ep_lens(E), o, g, a, device="cuda")
    dev = DeviceHerReplayBuffer(label, horizon=T, goal_selection_strategy="final", reward_fn=label.compute_reward, seed=3)
    assert dev.ring.numel() > 2 ** 31 and dev.record_floats == 156
    dev.clock[0] = T - 1                                            # the next add lands in the last slot ...
    dev.ep_start.fill_(T - 2)                                       # ... and closes a two-step episode in every env
    r = lambda *s: torch.rand(*s, device="cuda")
    obs = {"observation": r(E, o), "achieved_goal": r(E, g), "desired_goal": r(E, g)}
    nxt = {"observation": r(E, o), "achieved_goal": r(E, g)}
    act, rew = r(E, a), r(E)
    dev.add(obs, nxt, act, rew, torch.ones(E, device="cuda", dtype=torch.uint8))
    rec = dev.ring[T - 1]
    expect = torch.cat([obs["observation"], nxt["observation"], obs["achieved_goal"], nxt["achieved_goal"], obs["desired_goal"], act,
                        rew[:, None], torch.ones(E, 1, device="cuda")], 1)
    assert torch.equal(rec, expect) and not bool(dev.ring[:T - 1].any())
    assert bool((dev.ep_end[T - 2:] == T - 1).all()) and bool((dev.ep_first[T - 2:] == T - 2).all()) and bool((dev.ep_end[:T - 2] == -1).all())
    assert dev.t == T and bool((dev.ep_start == T).all())
    # every older entry becomes a closed one-step episode, and every record names its slot and env
    own = torch.arange(T - 2, device="cuda")[:, None].expand(T - 2, E)
    dev.ep_end[:T - 2], dev.ep_first[:T - 2] = own, own
    slot = torch.arange(T, device="cuda", dtype=torch.float32)[:, None]
    dev.ring[:, :, 0], dev.ring[:, :, 1] = slot, torch.arange(E, device="cuda", dtype=torch.float32)[None, :]
    dev.ring[:, :, 2 * o + g] = slot + 0.5                          # next_achieved_goal[0]
    b = dev.sample(4096)
    assert bool(b["ok"].all())
    far = b["time"] * E * 156 >= 2 ** 31
    assert int(far.sum()) > 400                                     # ~18 % of the rows lie past 2^31 floats
    assert torch.equal(b["observation"][:, 0], b["time"].to(torch.float32)) and torch.equal(b["observation"][:, 1], b["env"].to(torch.float32))
    rel = b["relabelled"]
    assert torch.equal(b["desired_goal"][rel][:, 0], b["goal_time"][rel].to(torch.float32) + 0.5)
    assert torch.equal(b["goal_time"], dev.ep_end[b["time"], b["env"]])
