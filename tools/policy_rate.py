#!/usr/bin/env python3
"""Time the rollout's policy evaluation with device events: train.py's torch chain - `model.dist(x).sample().clamp(-1, 1)` plus
`model.value(x)` under no_grad - against device_policy.py's DevicePolicy.act_into (one HIP launch and the counter tick, all four
outputs).  Median of 3 warmed windows of 50 calls per leg.

  python tools/policy_rate.py [--out profiles/policy_rate.json] [--rows 4096 65536]

Reach widths (8 + 3 + 3) and PickAndPlace widths (24 + 3 + 3), act_dim 4, at 4 096 and 65 536 rows.  Both legs read the same
normalised [rows, D] tensor and the same ActorCritic.  Legs per size and width, in this order: torch, hip, torch again (drift).
`hip_actions_only` is act_into without logp / value (the rollout's own call: the value tower is skipped).  `torch_launches` is the
number of kernels the torch chain enqueues per call, counted with the torch profiler after the last timed window of the run (a
tracer slows the host: nothing is timed once it has been started)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_xarm_amd.device_policy import DevicePolicy  # noqa: E402
from gym_xarm_amd.train import ActorCritic  # noqa: E402

CALLS = 50
WIDTHS = {"XarmReach-v0": (8, 3), "XarmPDPickAndPlace-v0": (24, 3)}
ACT_DIM = 4


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


def count_launches(fn):
    """device kernels of one call; None when the profiler is not usable here"""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA)
    except Exception as ex:
        print("launch count unavailable: %r" % (ex,), file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, nargs="+", default=[4096, 65536])
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "calls_per_window": CALLS, "act_dim": ACT_DIM, "legs": []}
    for env_id, (od, gd) in WIDTHS.items():
        D = od + 2 * gd
        for E in args.rows:
            torch.manual_seed(0)
            model = ActorCritic(D, ACT_DIM).cuda()
            x = (torch.rand(E, D, device="cuda") * 2 - 1) * 3
            pol = DevicePolicy(model, seed=0)
            out = pol.alloc_out(E)
            act_only = {k: out[k] for k in ("action", "env_action")}

            def torch_call():
                with torch.no_grad():
                    a = model.dist(x).sample().clamp(-1, 1)
                    v = model.value(x)
                return a, v

            def hip_call():
                pol.act_into(out, x)

            def hip_actions_only():
                pol.act_into(act_only, x)

            for _ in range(2 * CALLS):
                torch_call()
                hip_call()
            for impl, fn in (("torch_first", torch_call), ("hip", hip_call), ("hip_actions_only", hip_actions_only), ("torch_last", torch_call)):
                ms = timed(fn, CALLS)
                res["legs"].append(dict(widths=env_id, obs_dim=od, goal_dim=gd, rows=E, impl=impl, ms_per_call=ms))
                print(json.dumps(res["legs"][-1]), flush=True)
            last = (torch_call, hip_call)
    res["torch_launches"], res["hip_launches"] = count_launches(last[0]), count_launches(last[1])
    print(json.dumps({"torch_launches": res["torch_launches"], "hip_launches": res["hip_launches"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
