#!/usr/bin/env python3
"""Time the two HER replay buffers of gym_xarm_amd/her.py with device events: median of 3 warmed windows per leg.

  python tools/her_rate.py [--out profiles/her_rate.json] [--envs 65536 4096]

PickAndPlace dimensions, horizon 200, at 65 536 and at 4 096 envs.  Both buffers are fed the same synthetic stream: random
rows, and a done mask that closes env e's episode every 50th call ((e + t) % 50 == 0 - the steady state of 50-step episodes
that are out of phase, E / 50 closing per call), 100 calls before anything is timed.  Legs per size, in this order: the torch
HerReplayBuffer's add, sample(4 096), sample(65 536); DeviceHerReplayBuffer's add, sample_into of 4 096 and 65 536 rows (two
launches + the reward kernel); then the torch legs again, to show drift.  A window is 50 adds (one full cycle of the done masks)
or 20 samples.  The torch sample reads a count back per call (nonzero), so its event time includes that host round trip - it
is what a training loop would wait for.
Kernel times of their own: rocprofv3 --kernel-trace --stats -- python tools/her_rate.py (profiles/README.md)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_xarm_amd  # noqa: E402
from gym_xarm_amd.her import DeviceHerReplayBuffer, HerReplayBuffer  # noqa: E402

HORIZON, EP_LEN = 200, 50


def timed(fn, iters, windows=3):
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
    return sorted(out)[len(out) // 2]


class Stream:
    """the synthetic transition stream; each buffer keeps its own position in it"""

    def __init__(self, env):
        E, dev = env.num_envs, env.device
        r = lambda *s: torch.rand(*s, device=dev)
        self.obs = {"observation": r(E, env.obs_dim), "achieved_goal": r(E, env.goal_dim), "desired_goal": r(E, env.goal_dim)}
        self.nxt = {"observation": r(E, env.obs_dim), "achieved_goal": r(E, env.goal_dim)}
        self.act, self.rew = r(E, env.act_dim), r(E)
        e = torch.arange(E, device=dev)
        self.done = [((e + t) % EP_LEN == 0).to(torch.uint8) for t in range(EP_LEN)]

    def feeder(self, buf):
        pos = [0]

        def add():
            buf.add(self.obs, self.nxt, self.act, self.rew, self.done[pos[0] % EP_LEN])
            pos[0] += 1
        return add


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, nargs="+", default=[65536, 4096])
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "horizon": HORIZON, "episode_length": EP_LEN, "legs": []}
    for E in args.envs:
        env = gym_xarm_amd.make("XarmPDPickAndPlace-v0", num_envs=E, seed=0)
        stream = Stream(env)
        tb = HerReplayBuffer(env, horizon=HORIZON, seed=0)
        db = DeviceHerReplayBuffer(env, horizon=HORIZON, seed=0)
        t_add, d_add = stream.feeder(tb), stream.feeder(db)
        for _ in range(2 * EP_LEN):
            t_add()
            d_add()
        assert tb.num_valid() == db.num_valid() > 0
        outs = {B: db.alloc_out(B) for B in (4096, 65536)}

        def leg(name, impl, fn, iters, rows=None):
            ms = timed(fn, iters)
            res["legs"].append(dict(envs=E, leg=name, impl=impl, rows=rows, ms=ms))
            print(json.dumps(res["legs"][-1]), flush=True)

        def torch_legs(tag):
            leg("add", tag, t_add, EP_LEN)
            for B in (4096, 65536):
                leg("sample", tag, lambda: tb.sample(B), 20, B)

        torch_legs("torch_first")
        leg("add", "hip", d_add, EP_LEN)
        for B in (4096, 65536):
            leg("sample", "hip", lambda: db.sample_into(outs[B]), 20, B)
        torch_legs("torch_last")
        assert bool(outs[65536]["ok"].all()) and int(db.fail_count.item()) == 0
        env.close()
        del tb, db, stream, outs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
