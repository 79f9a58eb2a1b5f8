#!/usr/bin/env python3
"""Time the uniform replay buffers of gym_xarm_amd/replay.py with device events: median, minimum and maximum of 5 warmed windows per leg.

  python tools/replay_rate.py [--out profiles/replay_rate.json] [--envs 256 4096 65536]

Two records - a record here is the observation and action widths of one env kind: Handover NoGoal (flat, 29 + 8) and PickAndPlace
(25 + 2 x 3, 4) - at 256, 4 096 and 65 536 envs with buffer_size 1 000 000, batches of 256 and 4 096 rows.  No env steps: both
buffers are fed the same synthetic stream (random rows; env e finishes every 50th call, (e + t) % 50 == 0, every other one of those
by the time limit), 100 calls before anything is timed.  Legs per size, in this order: the torch ReplayBuffer's add, sample and
sample + normalisation (sac.flat_batch); DeviceReplayBuffer's add, sample_into without and with `normalize`; then the torch legs
again, to show drift.  A window is 50 adds or 50 samples; every leg runs on the current stream.

`update_from`: on one 256-env PickAndPlace env, DeviceSAC (64-64 tanh) and DeviceTD3 (64-64 tanh), 256 rows: update_from on a
DeviceReplayBuffer against update_from on a DeviceHerReplayBuffer - the HER composition: sample, tick, reward kernel, ok multiply, two
normaliser launches, two copies - on the same model, and `update` alone on a resident batch.  `launches` is the number of kernels each
call enqueues, counted with the torch profiler after the last timed window of the run (nothing is timed once a tracer has run).
Kernel times of their own: rocprofv3 --kernel-trace --stats -- python tools/replay_rate.py (profiles/README.md)."""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gym_xarm_amd  # noqa: E402
from gym_xarm_amd import sac as S  # noqa: E402
from gym_xarm_amd.normalize import DeviceVecNormalize  # noqa: E402
from gym_xarm_amd.replay import DeviceReplayBuffer, ReplayBuffer  # noqa: E402
from sac_rate import count_launches  # noqa: E402

RECORDS = {"handover_nogoal": dict(obs_dim=29, goal_dim=0, act_dim=8), "pick_and_place": dict(obs_dim=25, goal_dim=3, act_dim=4)}
EP_LEN, BUFFER_SIZE = 50, 1_000_000


def timed(fn, iters, windows=5):
    """(median, min, max) ms per call over `windows` windows of `iters` calls, after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def widths_env(E, obs_dim, goal_dim, act_dim):
    """what the buffers and the normaliser read of an env: its widths"""
    return types.SimpleNamespace(num_envs=E, device=torch.device("cuda"), obs_dim=obs_dim, goal_dim=goal_dim, act_dim=act_dim, action_dim=act_dim,
                                 flat_observation=goal_dim == 0)


class Stream:
    """the synthetic transition stream; each buffer keeps its own position in it"""

    def __init__(self, env):
        E, dev = env.num_envs, env.device
        r = lambda *s: torch.rand(*s, device=dev)
        if env.goal_dim == 0:
            self.obs, self.nxt = r(E, env.obs_dim), r(E, env.obs_dim)
        else:
            self.obs = {"observation": r(E, env.obs_dim), "achieved_goal": r(E, env.goal_dim), "desired_goal": r(E, env.goal_dim)}
            self.nxt = {"observation": r(E, env.obs_dim), "achieved_goal": r(E, env.goal_dim)}
        self.act, self.rew = r(E, env.act_dim), r(E)
        e = torch.arange(E, device=dev)
        self.done = [((e + t) % EP_LEN == 0).to(torch.uint8) for t in range(EP_LEN)]
        self.timeout = [d & (e % 2 == 0).to(torch.uint8) for d in self.done]

    def feeder(self, buf, her=False):
        pos = [0]

        def add():
            k = pos[0] % EP_LEN
            if her:
                buf.add(self.obs, self.nxt, self.act, self.rew, self.done[k])
            else:
                buf.add(self.obs, self.nxt, self.act, self.rew, self.done[k], self.timeout[k])
            pos[0] += 1
        return add


def buffer_legs(res, name, dims, E):
    env = widths_env(E, **dims)
    stream = Stream(env)
    venv = DeviceVecNormalize(env, monitor_capacity=max(E, 1))
    venv.stats[:venv.dim] = 0.5
    tb, db = ReplayBuffer(env, BUFFER_SIZE, seed=0), DeviceReplayBuffer(env, BUFFER_SIZE, seed=0)
    t_add, d_add = stream.feeder(tb), stream.feeder(db)
    for _ in range(2 * EP_LEN):
        t_add()
        d_add()
    outs = {B: db.alloc_out(B) for B in (256, 4096)}

    def leg(what, impl, fn, iters, rows=None):
        ms, lo, hi = timed(fn, iters)
        res["legs"].append(dict(record=name, envs=E, horizon=db.horizon, leg=what, impl=impl, rows=rows, ms=ms, ms_min=lo, ms_max=hi))
        print(json.dumps(res["legs"][-1]), flush=True)

    def torch_legs(tag):
        leg("add", tag, t_add, EP_LEN)
        for B in (256, 4096):
            leg("sample", tag, lambda: tb.sample(B), 50, B)
            leg("sample_normalize", tag, lambda: S.flat_batch(venv, tb.sample(B)), 50, B)

    torch_legs("torch_first")
    leg("add", "hip", d_add, EP_LEN)
    for B in (256, 4096):
        leg("sample", "hip", lambda: db.sample_into(outs[B]), 50, B)
        leg("sample_normalize", "hip", lambda: db.sample_into(outs[B], venv), 50, B)
    torch_legs("torch_last")
    assert bool(outs[4096]["use"].all())
    del tb, db, stream, outs, venv
    torch.cuda.empty_cache()


def update_legs(res, B=256, E=256):
    from gym_xarm_amd.device_sac import DeviceSAC
    from gym_xarm_amd.device_td3 import DeviceTD3
    from gym_xarm_amd.her import DeviceHerReplayBuffer
    from gym_xarm_amd.td3 import Td3Policy
    env = gym_xarm_amd.make("XarmPDPickAndPlace-v0", num_envs=E, seed=0)
    stream = Stream(env)
    venv = DeviceVecNormalize(env, monitor_capacity=max(E, 1))
    her, uni = DeviceHerReplayBuffer(env, horizon=200, seed=0), DeviceReplayBuffer(env, BUFFER_SIZE, seed=0)
    h_add, u_add = stream.feeder(her, her=True), stream.feeder(uni)
    for _ in range(2 * EP_LEN):
        h_add()
        u_add()
    torch.manual_seed(0)
    learners = {"sac": DeviceSAC(S.SacPolicy(venv.dim, env.action_dim).cuda(), B), "td3": DeviceTD3(Td3Policy(venv.dim, env.action_dim).cuda(), B)}
    keep = []
    for algo, d in learners.items():
        d.update_from(uni, venv)
        batch = {"obs": d.buffers["obs"], "next_obs": d.buffers["next_obs"], "action": d._uniform_sample["action"].clone(),
                 "reward": d._uniform_sample["reward"].clone(), "done": d.buffers["done"], "use": d.buffers["use"]}
        calls = (("update", lambda d=d, batch=batch: d.update(batch)), ("update_from_uniform", lambda d=d: d.update_from(uni, venv)),
                 ("update_from_her", lambda d=d: d.update_from(her, venv)))
        for what, fn in calls + calls[:1]:
            ms, lo, hi = timed(fn, 50)
            res["update_from"].append(dict(algo=algo, net_arch=[64, 64], rows=B, call=what, stated_update_launches=d.launches, ms=ms, ms_min=lo, ms_max=hi))
            print(json.dumps(res["update_from"][-1]), flush=True)
        keep.append((algo, calls))
    for algo, calls in keep:        # a tracer slows the host: counted after every timed window
        res["launches"].append(dict(algo=algo, **{what: count_launches(fn) for what, fn in calls}))
        print(json.dumps(res["launches"][-1]), flush=True)
    env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 4096, 65536])
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "buffer_size": BUFFER_SIZE, "episode_length": EP_LEN, "records": RECORDS, "legs": [],
           "update_from": [], "launches": []}
    for name, dims in RECORDS.items():
        for E in args.envs:
            buffer_legs(res, name, dims, E)
    update_legs(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
