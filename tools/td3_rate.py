#!/usr/bin/env python3
"""Time one TD3 step with device events: the torch block of gym_xarm_amd/td3.py (td3_step on a Td3Policy(net_arch, activation)) against
device_td3.py's DeviceTD3.update (7 n_hidden + 14 HIP launches).  Median of 3 warmed windows per leg.

  python tools/td3_rate.py [--out profiles/td3_rate.json] [--batch 256 4096 65536] [--commit ID] [--learn] [--learn-steps 12000]

Shapes [256, 256, 256] ReLU and [256, 256] tanh, at Reach widths (14 columns) and PickAndPlace widths (30), act_dim 4, batches of 256,
4 096 and 65 536 rows, policy_delay 1 and 2.  Both legs read the same batch and start from the same Td3Policy; each steps its own copy
and draws its own noise.  Legs per case, in this order: torch, hip, torch again (drift): `spread` is |torch_last - torch_first| /
torch_first.  A window is 20 steps (6 at 65 536 rows): an even count, so with policy_delay 2 exactly half of any window's steps carry the
actor phase, in both legs.  `launches`: per shape, the kernels one step of the torch block (`torch`, a step with an actor update) and of
`update` (`hip`) enqueue at 256 rows and Reach widths, counted with the torch profiler after the last timed window of the run (nothing is
timed once a tracer has run), beside `DeviceTD3.launches` (`hip_stated`).
--learn: sparse Reach with HER, 256 envs, one TD3 step of 256 rows per env step, [256, 256, 256] ReLU - the torch block once and the
device path (device_update + device_normalize) once, in this order, with both success curves, wall times and end-to-end env steps/s."""
import argparse
import copy
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_xarm_amd.device_td3 import DeviceTD3  # noqa: E402
from gym_xarm_amd.td3 import Td3Policy, make_optimizers, td3_step, train_td3  # noqa: E402
from sac_rate import count_launches, timed  # noqa: E402

WIDTHS = {"XarmReach-v0": 14, "XarmPDPickAndPlace-v0": 30}
SHAPES = (((256, 256, 256), "relu"), ((256, 256), "tanh"))
DELAYS = (1, 2)
ACT_DIM = 4


def learn(steps):
    out = {"env": "XarmReach-v0", "reward_type": "sparse", "num_envs": 256, "steps": steps, "batch_size": 256, "net_arch": [256, 256, 256], "activation": "relu",
           "log_every": 1000}
    for name, kw in (("torch", {}), ("hip", dict(device_update=True, device_normalize=True))):
        t0 = time.perf_counter()
        _, _, hist = train_td3("XarmReach-v0", config={"reward_type": "sparse", "GUI": False}, num_envs=256, steps=steps, batch_size=256,
                               log_every=1000, quiet=True, net_arch=(256, 256, 256), activation="relu", **kw)
        wall = time.perf_counter() - t0
        out[name] = {"success_rate": [r["success_rate"] for r in hist], "wall_s": wall, "env_steps_per_sec": steps * 256 / wall}
        print(json.dumps({name: out[name]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--commit", default=None, help="recorded in the JSON: the commit the figures were taken at")
    ap.add_argument("--learn", action="store_true")
    ap.add_argument("--learn-only", action="store_true", help="--learn without the timed legs")
    ap.add_argument("--learn-steps", type=int, default=12000)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "act_dim": ACT_DIM, "legs": []}
    keep = []
    for arch, act in (() if args.learn_only else SHAPES):
        for env_id, D in WIDTHS.items():
            for B in args.batch:
                for delay in DELAYS:
                    calls = 6 if B > 4096 else 20
                    torch.manual_seed(0)
                    model_t = Td3Policy(D, ACT_DIM, arch, act).cuda()
                    model_h = copy.deepcopy(model_t)
                    opts = make_optimizers(model_t)
                    td3 = DeviceTD3(model_h, B, policy_delay=delay)
                    batch = {"obs": (torch.rand(B, D, device="cuda") * 2 - 1) * 3, "next_obs": (torch.rand(B, D, device="cuda") * 2 - 1) * 3,
                             "action": torch.rand(B, ACT_DIM, device="cuda") * 2 - 1, "reward": -(torch.rand(B, device="cuda") < 0.8).float(),
                             "done": (torch.rand(B, device="cuda") < 0.04).float(), "use": torch.ones(B, device="cuda")}
                    count = {"n": 0, "last": None}

                    def torch_call(model_t=model_t, opts=opts, batch=batch, count=count, delay=delay):
                        count["n"] += 1
                        count["last"] = td3_step(model_t, opts, batch, count["n"], policy_delay=delay, last=count["last"])

                    def hip_call(td3=td3, batch=batch):
                        td3.update(batch)

                    for _ in range(2):
                        torch_call()
                        hip_call()
                    ms = {}
                    tag = dict(net_arch=list(arch), activation=act, widths=env_id, obs_width=D, batch=B, policy_delay=delay, steps_per_window=calls)
                    for impl, fn in (("torch_first", torch_call), ("hip", hip_call), ("torch_last", torch_call)):
                        ms[impl] = timed(fn, calls)
                        res["legs"].append(dict(tag, impl=impl, ms_per_step=ms[impl]))
                        print(json.dumps(res["legs"][-1]), flush=True)
                    res["legs"].append(dict(tag, impl="ratio", torch_over_hip=min(ms["torch_first"], ms["torch_last"]) / ms["hip"],
                                            spread=abs(ms["torch_last"] - ms["torch_first"]) / ms["torch_first"]))
                    print(json.dumps(res["legs"][-1]), flush=True)
                    if B == min(args.batch) and env_id == next(iter(WIDTHS)) and delay == 1:
                        keep.append((torch_call, hip_call, td3.launches, dict(net_arch=list(arch), activation=act, widths=env_id, batch=B, policy_delay=delay)))
    if args.learn or args.learn_only:
        res["learn"] = learn(args.learn_steps)
    res["launches"] = [dict(k[3], torch=count_launches(k[0]), hip=count_launches(k[1]), hip_stated=k[2]) for k in keep]
    print(json.dumps({"launches": res["launches"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
