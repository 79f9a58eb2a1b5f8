#!/usr/bin/env python3
"""Time the per-step bookkeeping of the training driver with device events: train.py's torch VecNormalize.step +
EpisodeMonitor.update against normalize.py's DeviceVecNormalize.step_into (three HIP launches).  Median of 3 warmed windows per leg.

  python tools/norm_rate.py [--out profiles/norm_rate.json] [--envs 4096 65536]

PickAndPlace widths (24 + 3 + 3) and Reach widths (8 + 3 + 3) at 4 096 and 65 536 envs.  Both classes are fed the same synthetic
env outputs: random rows and rewards, and a done mask that ends env e's episode every 50th call ((e + t) % 50 == 0: E / 50 envs
finish per call), through a stand-in env whose step only hands out those tensors - the env's own kernels are not in the timing.
Legs per size and width, in this order: torch, hip, torch again (drift).  A window is 50 calls, one cycle of the done masks.
`ratio_to_env_step` divides a leg's ms per call by that env's own step time from the README table (ENV_STEP_MS below); sizes the
table does not list carry null."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_xarm_amd.normalize import DeviceVecNormalize  # noqa: E402
from gym_xarm_amd.train import EpisodeMonitor, VecNormalize  # noqa: E402

EP_LEN = 50
WIDTHS = {"XarmPDPickAndPlace-v0": (24, 3), "XarmReach-v0": (8, 3)}
# README.md, the table under 'One MI355X': ms per env.step call of the batch.  Reach: its one step kernel; PickAndPlace: envs /
# (env steps/s), step and in-call reset kernels together (65 536 / 1.60e7, 4 096 / 1.39e6).  Reach at 65 536 is not in the table.
ENV_STEP_MS = {("XarmReach-v0", 4096): 0.57, ("XarmPDPickAndPlace-v0", 65536): 4.10, ("XarmPDPickAndPlace-v0", 4096): 2.95}


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


class SyntheticEnv:
    """hands the same [E, .] tensors out on every step; only the done mask moves"""

    def __init__(self, E, obs_dim, goal_dim, device):
        self.num_envs, self.obs_dim, self.goal_dim, self.act_dim, self.device = E, obs_dim, goal_dim, 4, torch.device(device)
        r = lambda *s: torch.rand(*s, device=device) * 2 - 1
        self.obs = {"observation": r(E, obs_dim), "achieved_goal": r(E, goal_dim), "desired_goal": r(E, goal_dim)}
        self.rew = r(E)
        e = torch.arange(E, device=device)
        self.done = [((e + t) % EP_LEN == 0).to(torch.uint8) for t in range(EP_LEN)]
        self.t = 0

    def reset(self):
        return self.obs

    def step(self, actions):
        self.t += 1
        return self.obs, self.rew, self.done[self.t % EP_LEN], {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "episode_length": EP_LEN, "calls_per_window": EP_LEN, "legs": []}
    for env_id, (od, gd) in WIDTHS.items():
        for E in args.envs:
            te, de = SyntheticEnv(E, od, gd, "cuda"), SyntheticEnv(E, od, gd, "cuda")
            tv, tm = VecNormalize(te), EpisodeMonitor(E, te.device)
            dv = DeviceVecNormalize(de)
            out = dv.alloc_out()
            tv.reset()
            dv.reset()

            def torch_call():
                nobs, nrew, done, info, raw = tv.step(None)
                tm.update(raw, done)

            def hip_call():
                obs, rew, done, info = de.step(None)
                dv.step_into(out, obs, rew, done, None)

            for _ in range(2 * EP_LEN):
                torch_call()
                hip_call()
            assert tm.n == dv.monitor.n > 0
            step_ms = ENV_STEP_MS.get((env_id, E))
            for impl, fn in (("torch_first", torch_call), ("hip", hip_call), ("torch_last", torch_call)):
                ms = timed(fn, EP_LEN)
                res["legs"].append(dict(widths=env_id, obs_dim=od, goal_dim=gd, envs=E, impl=impl, ms_per_call=ms,
                                        env_step_ms=step_ms, ratio_to_env_step=None if step_ms is None else ms / step_ms))
                print(json.dumps(res["legs"][-1]), flush=True)
            del tv, tm, dv, te, de, out
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
