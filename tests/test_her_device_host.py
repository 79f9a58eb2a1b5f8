"""The device-resident HER buffer's core (gym_xarm_amd/csrc/xarm_her_core.h) on the CPU: the g++ build (tests/her_host.py) against
the torch HerReplayBuffer of gym_xarm_amd/her.py on CPU tensors, fed the same scripted stream - bookkeeping after every add,
every sampled row traced back to the checker's storage, the distribution of the rejection sampler, the 64-try cap,
determinism - and the argument checks of the three C-ABI entry points through the real library (no device needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import her_host as HH
from gym_xarm_amd.her import HerReplayBuffer, collect

STRATEGIES = ("future", "final", "episode")
LENS = HH.ep_lens(7)            # 3, 4, 5, 5, 2, 4 and one env of length 1


def scripted_pair(horizon, steps=40, after_add=None):
    env = HH.ScriptedEnv(LENS)
    chk = HerReplayBuffer(env, horizon=horizon, n_sampled_goal=4, seed=0)
    host = HH.HostHer(env.num_envs, horizon, env.obs_dim, env.goal_dim, env.act_dim, seed=11)
    tee = HH.Tee([chk, host], after_add and (lambda n: after_add(n, chk, host)))
    collect(env, tee, env.policy, steps)
    return chk, host


@pytest.fixture(scope="module")
def state40():
    """40 steps into a ring of 12 slots: wrapped three times.  Shared and only read (sampling advances the host clock's
    sample_calls, which every test sets itself)."""
    return scripted_pair(12)


def first_time(t, e):
    """first absolute time of the episode of env e that holds time t, from the script"""
    L = np.asarray(LENS)[e]
    return (t // L) * L


@pytest.mark.parametrize("horizon", [10, 12])      # 2 * max_len exactly, and the 12 of tests/test_her.py
def test_bookkeeping_matches_the_torch_buffer_after_every_add(horizon):
    seen = []

    def compare(n, chk, host):
        assert host.clock[0] == n == chk.t
        assert np.array_equal(host.ep_end, chk.ep_end.numpy()), n
        assert np.array_equal(host.ep_start, chk.ep_start.numpy()), n
        closed = host.ep_end >= 0
        slot_time = chk.slot_time.numpy()[:, None].repeat(host.E, 1)
        env_of = np.arange(host.E)[None, :].repeat(horizon, 0)
        assert np.array_equal(host.ep_first[closed], first_time(slot_time[closed], env_of[closed])), n
        assert bool((host.ep_first[~closed & (slot_time < 0)] == -1).all())
        seen.append(int(closed.sum()))

    chk, host = scripted_pair(horizon, after_add=compare)
    assert len(seen) == 40 and seen[0] == 1 and seen[-1] > 0     # step 1 closes the length-1 env's episode only
    R = host.ring
    o, g = 4, 3
    for name, lo, hi in (("obs", 0, o), ("next_obs", o, 2 * o), ("ag", 2 * o, 2 * o + g), ("next_ag", 2 * o + g, 2 * o + 2 * g),
                         ("dg", 2 * o + 2 * g, 2 * o + 3 * g), ("act", 2 * o + 3 * g, 2 * o + 3 * g + 2)):
        assert np.array_equal(R[:, :, lo:hi], getattr(chk, name).numpy()), name
    assert np.array_equal(R[:, :, -2], chk.rew.numpy()) and np.array_equal(R[:, :, -1] != 0, chk.done.numpy())


def check_rows(out, chk, host, strategy):
    """every ok row of `out` against the checker's storage; every failed row all zero.  Returns the ok mask."""
    T, t_now = chk.horizon, chk.t
    ok = out["ok"].astype(bool)
    e, t, tg = out["env"], out["time"], out["goal_time"]
    for k, _, _ in HH.OUT:
        assert not out[k][~ok].any(), "failed row not zero: %s" % k
    s = t % T
    slot_time, ep_end = chk.slot_time.numpy(), chk.ep_end.numpy()
    valid = chk._valid().numpy()
    E = chk.E
    assert bool(((e >= 0) & (e < E))[ok].all())
    assert np.array_equal(slot_time[s][ok], t[ok]), "row from an overwritten slot"
    assert bool(valid[s, e][ok].all()) and bool((ep_end[s, e][ok] >= 0).all()), "row from a running episode"
    for k, store in (("observation", chk.obs), ("next_observation", chk.next_obs), ("achieved_goal", chk.ag),
                     ("next_achieved_goal", chk.next_ag), ("action", chk.act), ("reward", chk.rew)):
        assert np.array_equal(out[k][ok], store.numpy()[s, e][ok]), k
    assert np.array_equal(out["done"][ok] != 0, chk.done.numpy()[s, e][ok])
    n_her = out["n_her"]
    rel = np.arange(len(e)) < n_her
    end, first = ep_end[s, e], first_time(t, e)
    assert np.array_equal(host.ep_first[s, e][ok], first[ok])
    sg = tg % T
    assert np.array_equal(slot_time[sg][ok], tg[ok]), "goal from an overwritten slot"
    assert np.array_equal(out["desired_goal"][ok & rel], chk.next_ag.numpy()[sg, e][ok & rel])
    assert np.array_equal(out["desired_goal"][ok & ~rel], chk.dg.numpy()[s, e][ok & ~rel])
    # the relabelled rows come first: hindsight goals are achieved goals (first component = env id >= 0), stored ones are < 0
    assert bool((out["desired_goal"][ok & rel][:, 0] >= 0).all()) and bool((out["desired_goal"][ok & ~rel][:, 0] < 0).all())
    assert bool((tg <= end)[ok].all())
    if strategy == "episode":                      # anywhere in the part of the episode the ring still holds
        assert bool((tg >= np.maximum(first, t_now - T))[ok].all())
    else:
        assert bool((tg >= t)[ok].all())
    if strategy == "final":
        assert np.array_equal(tg[ok], end[ok])
    assert np.array_equal(ep_end[sg, e][ok], end[ok]), "goal from another episode"
    return ok


def valid_share(chk):
    stored = min(chk.t, chk.horizon) * chk.E
    return float(chk._valid().sum()) / stored


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_rows_trace_back_to_the_checkers_storage(state40, strategy):
    chk, host = state40
    assert valid_share(chk) >= 0.25                # all-ok below is then a < 500 * 0.75^64 = 5e-6 claim
    host.clock[1] = 3
    out = host.sample(500, strategy)
    assert out["n_her"] == 400 == round(0.8 * 500)
    ok = check_rows(out, chk, host, strategy)
    assert ok.all() and host.clock[1] == 4
    span = (out["goal_time"] - out["time"])
    if strategy == "future":
        assert span.max() == 4 and span.min() == 0
    if strategy == "episode":
        assert span.min() < 0 < span.max()


def within(counts, n, p, what):
    """every count within 5 binomial sigma of n p"""
    sigma = np.sqrt(n * p * (1 - p))
    z = np.abs(np.asarray(counts) - n * p) / np.maximum(sigma, 1e-12)
    assert float(z.max()) <= 5.0, "%s: %.2f sigma" % (what, float(z.max()))


def test_rejection_sampling_is_uniform_over_valid_entries_and_future_offsets(state40):
    chk, host = state40
    assert valid_share(chk) >= 0.25
    B = 60000
    host.clock[1] = 0
    out = host.sample(B, "future")
    assert out["ok"].all()
    valid = chk._valid().numpy()
    T, E = valid.shape
    counts = np.bincount((out["time"] % T) * E + out["env"], minlength=T * E).reshape(T, E)
    assert counts[~valid].sum() == 0
    within(counts[valid], B, 1.0 / valid.sum(), "entries")
    # 'future': the offset goal_time - time is uniform on [0, m), m = the transitions left in the episode, this one included
    left = chk.ep_end.numpy()[out["time"] % T, out["env"]] - out["time"] + 1
    off = out["goal_time"] - out["time"]
    assert left.max() == 5
    for m in range(1, int(left.max()) + 1):
        sel = left == m
        c = np.bincount(off[sel], minlength=m)
        assert len(c) == m and sel.sum() > 1000
        within(c, int(sel.sum()), 1.0 / m, "future offsets, %d left" % m)
    # 'episode' with the same draws: uniform on the part of the episode still in the ring
    host.clock[1] = 0
    ep = host.sample(B, "episode")
    assert np.array_equal(ep["env"], out["env"]) and np.array_equal(ep["time"], out["time"])
    lo = np.maximum(first_time(ep["time"], ep["env"]), chk.t - T)
    width = chk.ep_end.numpy()[ep["time"] % T, ep["env"]] - lo + 1
    for m in range(1, int(width.max()) + 1):
        sel = width == m
        if sel.sum():
            within(np.bincount((ep["goal_time"] - lo)[sel], minlength=m), int(sel.sum()), 1.0 / m, "episode offsets, width %d" % m)


def test_empty_buffer_fails_every_row():
    host = HH.HostHer(7, 12, 4, 3, 2)
    out = host.sample(50)
    for k, _, _ in HH.OUT:
        assert not out[k].any(), k
    assert host.fail_count[0] == 50 and host.clock[1] == 1


def test_try_cap_on_a_sparse_buffer():
    """one closed two-step episode among 12 stored entries: a row fails with probability (10 / 12)^64 = 8.6e-6, and whether or
    not one does, ok rows are right and failed rows are zero and counted"""
    env = HH.ScriptedEnv([6, 6])
    chk = HerReplayBuffer(env, horizon=12)
    host = HH.HostHer(2, 12, 4, 3, 2, seed=5)
    obs = env.reset()
    for t in range(6):
        env.t += 1
        nxt = env._obs()
        done = torch.tensor([t == 1, False])
        for b in (chk, host):
            b.add(obs, nxt, env.policy(obs), torch.tensor([0.5 + t, -t]), done)
        obs = nxt
    assert int(chk._valid().sum()) == 2 and min(chk.t, chk.horizon) * chk.E == 12
    out = host.sample(500, "future")
    ok = check_rows(out, chk, host, "future")
    assert host.fail_count[0] == (~ok).sum()
    assert ok.sum() >= 490 and set(out["time"][ok]) == {0, 1} and set(out["env"][ok]) == {0}


def test_same_seed_and_call_count_give_the_same_batch(state40):
    _, host = state40
    host.clock[1] = 9
    a = host.sample(300)
    b = host.sample(300)                           # sample_calls = 10
    host.clock[1] = 9
    c = host.sample(300)
    for k, _, _ in HH.OUT:
        assert np.array_equal(a[k], c[k]), k
    assert not np.array_equal(a["time"] * 64 + a["env"], b["time"] * 64 + b["env"])
    other = HH.HostHer(host.E, host.T, 4, 3, 2, seed=12)
    other.ring, other.ep_end, other.ep_first, other.clock = host.ring, host.ep_end, host.ep_first, np.array([host.clock[0], 9])
    d = other.sample(300)
    assert not np.array_equal(a["time"] * 64 + a["env"], d["time"] * 64 + d["env"])


def test_abi_argument_errors():
    from gym_xarm_amd import _native
    L = _native.load()
    lay = lambda *a: C.byref(_native.XarmHerLayout(*a))
    good = lay(7, 12, 4, 3, 2)
    err = lambda: L.xarm_last_error(None).decode()
    assert L.xarm_her_record_floats(good) == 2 * 4 + 3 * 3 + 2 + 2
    assert L.xarm_her_record_floats(lay(70, 200, 55, 12, 8)) == 156
    assert L.xarm_her_record_floats(None) == -1 and "NULL" in err()
    assert L.xarm_her_record_floats(lay(7, 1, 4, 3, 2)) == -1 and "horizon" in err()
    for bad in ((-1, 12, 4, 3, 2), (7, 12, 0, 3, 2), (7, 12, 4, 0, 2), (7, 12, 4, 3, 0)):
        assert L.xarm_her_record_floats(lay(*bad)) == -1, bad
        assert L.xarm_her_add(lay(*bad), *([None] * 14)) == -1, bad
        assert L.xarm_her_sample(lay(*bad), None, None, None, None, 0, 0, 4, 2, *([None] * 14)) == -1, bad
    assert L.xarm_her_add(good, *([None] * 14)) == -1 and "xarm_her_add: NULL pointer" in err()
    assert L.xarm_her_add(lay(0, 12, 4, 3, 2), *([None] * 14)) == 0            # no env: nothing to launch
    sample = lambda strategy, batch, n_her: L.xarm_her_sample(good, None, None, None, None, 0, strategy, batch, n_her, *([None] * 14))
    assert sample(0, 4, 5) == -1 and "n_her" in err()
    assert sample(0, 4, -1) == -1 and "n_her" in err()
    assert sample(0, -1, 0) == -1 and "batch" in err()
    assert sample(3, 4, 2) == -1 and "strategy" in err()
    assert sample(-1, 4, 2) == -1 and "strategy" in err()
    assert sample(0, 4, 2) == -1 and "xarm_her_sample: NULL pointer" in err()
    assert sample(2, 0, 0) == 0                                                # batch == 0: nothing to launch


def test_device_class_refuses_a_host_env_and_an_unknown_strategy():
    from gym_xarm_amd.her import DeviceHerReplayBuffer
    with pytest.raises(ValueError, match="GPU"):
        DeviceHerReplayBuffer(HH.ScriptedEnv(LENS))
    with pytest.raises(AssertionError):
        DeviceHerReplayBuffer(HH.ScriptedEnv(LENS), goal_selection_strategy="random")
