"""The uniform replay buffer's core (gym_xarm_amd/csrc/xarm_replay_core.h) on the CPU: the g++ build (tests/replay_host.py) against
the scripted stream's own arithmetic, NumPy's float64 normalisation and the torch class (gym_xarm_amd/replay.py ReplayBuffer), and the
training drivers on the torch block with a scripted flat env."""
import math

import numpy as np
import pytest
import torch

import replay_host as RH
from gym_xarm_amd.her import HerReplayBuffer
from gym_xarm_amd.replay import DeviceReplayBuffer, ReplayBuffer

FIELDS = ("obs", "next_obs", "action", "reward", "done", "use", "env", "time")


def make_env(kind, E):
    if kind == "flat":
        return RH.FlatScripted(RH.ep_lens(E), obs_dim=5, act_dim=3)       # odd D
    return RH.GoalScripted(RH.ep_lens(E), obs_dim=4, goal_dim=3, act_dim=2)


def pair(kind, E, T, steps, seed=0, handle_timeout=True):
    """(env, host build, torch class) after `steps` scripted steps into both buffers"""
    env = make_env(kind, E)
    host = RH.HostReplay(E, T, env.obs_dim, env.goal_dim, env.act_dim, seed=seed, handle_timeout=handle_timeout)
    ref = ReplayBuffer(env, buffer_size=T * E, handle_timeout_termination=handle_timeout, seed=seed)
    assert ref.horizon == T and ref.dim == host.D
    RH.collect(env, [host, ref], steps)
    return env, host, ref


def check_rows(kind, env, out, t, T):
    """every field of every row comes from the (env, time) the trace outputs name, and that time is in the ring"""
    e, tau = out["env"].astype(np.float64), out["time"].astype(np.float64)
    assert np.all(out["use"] == 1.0)
    assert np.all((out["time"] >= t - min(t, T)) & (out["time"] <= t - 1)) and np.all((out["env"] >= 0) & (out["env"] < env.num_envs))
    assert np.array_equal(out["obs"][:, 0], e) and np.array_equal(out["obs"][:, 1], tau)
    assert np.array_equal(out["next_obs"][:, 0], e) and np.array_equal(out["next_obs"][:, 1], tau + 1)
    assert np.array_equal(out["action"][:, 0], (e * 8 + 0.25 * tau).astype(np.float32))
    assert np.array_equal(out["reward"], (e / 4 - (tau + 1)).astype(np.float32))
    ends = np.array([(tt + 1) % RH.ep_lens(env.num_envs)[int(ee)] == 0 for ee, tt in zip(out["env"], out["time"])])
    assert np.array_equal(out["done"] != 0, ends & (out["env"] % 2 == 1))          # handling on: the terminated ones alone
    if kind == "goal":      # observation | achieved_goal | desired_goal; next: next_observation | next_achieved_goal | desired_goal
        o, g = env.obs_dim, env.goal_dim
        for k, dt in (("obs", 0), ("next_obs", 1)):
            assert np.array_equal(out[k][:, o], e) and np.array_equal(out[k][:, o + 1], tau + dt)
            assert np.array_equal(out[k][:, o + g], (-1.0 - e).astype(np.float32))


@pytest.mark.parametrize("kind", ["flat", "goal"])
@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("E", [1, 3, 7])
def test_rows_trace_to_one_transition_and_the_torch_class_replays_them(kind, E, T):
    for steps in (T - 1, 2 * T + 1):                     # before and after the ring wraps
        env, host, ref = pair(kind, E, T, steps)
        assert host.clock[0] == steps == ref.t
        out = host.sample(41)
        assert host.clock[1] == 1
        check_rows(kind, env, out, steps, T)
        mine = ref.sample(41, index=(out["time"] % T, out["env"]))
        for k in FIELDS:
            assert np.array_equal(mine[k].numpy(), out[k]), k
        own = ref.sample(41)                              # the class's own draw obeys the same invariants
        check_rows(kind, env, {k: v.numpy() for k, v in own.items()}, steps, T)


@pytest.mark.parametrize("kind", ["flat", "goal"])
def test_empty_buffer_gives_zero_rows_then_the_first_step(kind):
    env = make_env(kind, 3)
    host = RH.HostReplay(3, 4, env.obs_dim, env.goal_dim, env.act_dim)
    ref = ReplayBuffer(env, buffer_size=12)
    for out in (host.sample(9), {k: v.numpy() for k, v in ref.sample(9).items()}):
        for k in FIELDS:
            assert not out[k].any(), k
    RH.collect(env, [host, ref], 1)
    out = host.sample(9)
    assert np.all(out["time"] == 0) and np.all(out["use"] == 1)
    check_rows(kind, env, out, 1, 4)


def test_timeout_handling():
    for handle in (True, False):
        env, host, ref = pair("flat", 7, 12, 12, handle_timeout=handle)
        out = host.sample(300)
        lens = RH.ep_lens(7)
        ends = np.array([(t + 1) % lens[e] == 0 for e, t in zip(out["env"], out["time"])])
        trunc, term = ends & (out["env"] % 2 == 0), ends & (out["env"] % 2 == 1)
        assert trunc.any() and term.any() and (~ends).any()
        assert np.array_equal(out["done"] != 0, term if handle else ends)
        other = host.sample(300, handle_timeout=not handle)
        ends2 = np.array([(t + 1) % lens[e] == 0 for e, t in zip(other["env"], other["time"])])
        assert np.array_equal(other["done"] != 0, ends2 if handle else ends2 & (other["env"] % 2 == 1))
        mine = ref.sample(300, index=(out["time"] % 12, out["env"]))
        assert np.array_equal(mine["done"].numpy(), out["done"])
    # no flag given: nothing is a truncation
    env = make_env("flat", 3)
    host = RH.HostReplay(3, 8, env.obs_dim, 0, env.act_dim)
    obs = env.reset()
    for _ in range(8):
        prev = obs.clone()
        act = env.policy(prev)
        obs, rew, done, info = env.step(act)
        host.add(prev, obs, act, rew, done)
    out = host.sample(200)
    assert np.array_equal(out["done"] != 0, np.array([(t + 1) % RH.ep_lens(3)[e] == 0 for e, t in zip(out["env"], out["time"])]))


@pytest.mark.parametrize("kind", ["flat", "goal"])
def test_normalisation_is_numpys_float64_expression_rounded_once(kind):
    env, host, ref = pair(kind, 3, 5, 7)
    D, clip, eps = host.D, 10.0, 1e-8
    rng = np.random.default_rng(5)
    stats = np.zeros(2 * D + 4)
    stats[:D] = rng.normal(0.0, 500.0, D)
    stats[D:2 * D] = rng.uniform(0.5, 4e6, D)
    stats[D + 1] = 0.0              # var = 0: the denominator is sqrt(eps), the column clips at +-10
    stats[D + 2] = 1e-3             # a small variance: clips
    stats[D], stats[0] = 1e6, 2.75  # column 0 (the env index) stays inside the clip
    host.clock[1] = 0
    raw = host.sample(64)
    host.clock[1] = 0
    out = host.sample(64, stats=stats, clip_obs=clip, eps=eps)
    for k in ("obs", "next_obs"):
        want = np.clip((raw[k].astype(np.float64) - stats[:D]) / np.sqrt(stats[D:2 * D] + eps), -clip, clip).astype(np.float32)
        assert np.array_equal(out[k].view(np.uint32), want.view(np.uint32)), k
        assert np.all(np.abs(want[:, 1]) == clip) and np.all(np.abs(want[:, 0]) < clip) and np.any(np.abs(want[:, 2]) == clip)
    for k in ("action", "reward", "done", "use", "env", "time"):
        assert np.array_equal(out[k], raw[k]), k


def chi_square_bound(k, z=3.0902):
    """the 0.999 quantile of chi-square at k degrees of freedom by Wilson-Hilferty: k (1 - 2 / (9 k) + z sqrt(2 / (9 k)))^3"""
    return k * (1.0 - 2.0 / (9.0 * k) + z * math.sqrt(2.0 / (9.0 * k))) ** 3


def test_the_draw_is_uniform_over_the_stored_transitions():
    """chi-square of the counts over the T x E = 8 x 5 cells from 160 consecutive calls of 256 rows (seed 0) against draws / 40: the
    statistic is 55.4 (printed below), the bound 72.1 - the 0.999 quantile at 39 degrees of freedom by Wilson-Hilferty, derived and not
    measured"""
    env, host, ref = pair("flat", 5, 8, 11)
    counts = np.zeros((8, 5))
    for _ in range(160):
        out = host.sample(256)
        np.add.at(counts, (out["time"] % 8, out["env"]), 1)
    draws = 160 * 256
    assert counts.sum() == draws and host.clock[1] == 160
    stat = float(((counts - draws / 40) ** 2 / (draws / 40)).sum())
    bound = chi_square_bound(39)
    print("chi-square over 40 cells: %.2f (bound %.2f)" % (stat, bound))
    assert abs(bound - 72.1) < 0.1
    assert stat < bound


def test_rows_and_calls_draw_differently():
    env, host, ref = pair("flat", 7, 64, 64)
    a = host.sample(256)
    picks = lambda o: o["time"] * 7 + o["env"]
    assert len(np.unique(picks(a))) > 150                 # 256 draws from 448 cells: 195 distinct expected
    b = host.sample(256)
    assert np.mean(picks(a) == picks(b)) < 0.05
    for lo in (5, 2 ** 32 - 1):                           # the same low word below and above 2^32: the tag takes the high word
        host.clock[1] = lo
        x = host.sample(256)
        host.clock[1] = lo + 2 ** 32
        y = host.sample(256)
        assert np.mean(picks(x) == picks(y)) < 0.05
    host.clock[1] = 2 ** 32 - 1
    x = host.sample(256)
    assert host.clock[1] == 2 ** 32
    y = host.sample(256)
    assert np.mean(picks(x) == picks(y)) < 0.05
    other = RH.HostReplay(7, 64, 5, 0, 3, seed=1)
    other.ring[:], other.clock[:] = host.ring, (64, 0)
    host.clock[1] = 0
    assert np.mean(picks(other.sample(256)) == picks(host.sample(256))) < 0.05


def test_layout_errors_and_the_cpu_refusal():
    from gym_xarm_amd import _native
    L = RH.lib()
    import ctypes as C
    for bad in ((4, 0, 5, 0, 3), (4, 8, 0, 0, 3), (4, 8, 5, -1, 3), (4, 8, 5, 0, 0), (-1, 8, 5, 0, 3)):
        assert L.rh_record_floats(C.byref(_native.XarmReplayLayout(*bad))) == -1
    assert L.rh_record_floats(C.byref(_native.XarmReplayLayout(4, 8, 29, 0, 8))) == 2 * 29 + 8 + 3
    assert L.rh_record_floats(C.byref(_native.XarmReplayLayout(4, 1, 25, 3, 4))) == 2 * 31 + 4 + 3
    with pytest.raises(ValueError, match="ReplayBuffer is the torch implementation"):
        DeviceReplayBuffer(make_env("flat", 3))


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_drivers_train_on_a_flat_env_through_the_uniform_buffer(algo):
    from gym_xarm_amd import sac, td3
    train = sac.train_sac if algo == "sac" else td3.train_td3
    stats = sac.STATS if algo == "sac" else td3.STATS
    model, venv, hist = train(env=make_env("flat", 6), steps=30, learning_starts=5, batch_size=32, quiet=True, log_every=10, buffer_size=6 * 20)
    assert isinstance(venv.buffer, ReplayBuffer) and venv.buffer.t == 30 and venv.buffer.horizon == 20
    assert hist[-1]["updates"] == 25 and hist[-1]["step"] == 30
    assert all(math.isfinite(hist[-1][k]) for k in stats)
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert venv.buffer.timeout.any() and (venv.buffer.done & ~venv.buffer.timeout).any()      # the driver passed the truncation flag on


def test_driver_selects_the_buffer():
    from gym_xarm_amd import sac, td3
    with pytest.raises(ValueError, match="needs a goal env"):
        sac.train_sac(env=make_env("flat", 4), steps=3, replay="her", quiet=True)
    with pytest.raises(ValueError, match="needs a goal env"):
        td3.train_td3(env=make_env("flat", 4), steps=3, replay="her", quiet=True)
    with pytest.raises(ValueError, match="'her' or 'uniform'"):
        sac.train_sac(env=make_env("goal", 4), steps=3, replay="prioritised", quiet=True)
    model, venv, hist = sac.train_sac(env=make_env("goal", 4), steps=3, learning_starts=10, quiet=True)      # replay=None on a dict env: HER
    assert isinstance(venv.buffer, HerReplayBuffer) and venv.buffer.t == 3
    model, venv, hist = td3.train_td3(env=make_env("goal", 4), steps=12, learning_starts=4, batch_size=16, replay="uniform", quiet=True,
                                      buffer_size=40)
    assert isinstance(venv.buffer, ReplayBuffer) and venv.buffer.dim == 4 + 2 * 3 and hist[-1]["updates"] == 8
    assert all(math.isfinite(hist[-1][k]) for k in td3.STATS)


def test_cli_has_the_replay_options():
    from gym_xarm_amd import train
    with pytest.raises(SystemExit):
        train.main(["--algo", "a2c", "--replay", "uniform"])
    with pytest.raises(SystemExit):
        train.main(["--algo", "sac", "--replay", "prioritised"])
