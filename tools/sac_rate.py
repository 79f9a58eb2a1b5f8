#!/usr/bin/env python3
"""Time one SAC step with device events: the torch block of gym_xarm_amd/sac.py (sac_step: three autograd passes, three Adam.steps, the
Polyak loop) against device_sac.py's DeviceSAC.update (six HIP launches).  Median of 3 warmed windows of 20 steps per leg.

  python tools/sac_rate.py [--out profiles/sac_rate.json] [--batch 256 4096 65536] [--commit ID]

Batches of 256, 4 096 and 65 536 rows at Reach widths (14 columns) and PickAndPlace widths (30), act_dim 4.  Both legs read the same
batch and start from the same SacPolicy; each steps its own copy and draws its own noise.  Legs per size and width, in this order:
torch, hip, torch again (drift): `spread` is |torch_last - torch_first| / torch_first, the one spread this tool gives.
`torch_launches` is the number of kernels the torch leg enqueues per step, counted with the torch profiler after the last timed window
of the run (a tracer slows the host: nothing is timed once it has been started); `hip_launches` is counted the same way and
`hip_launches_update` is the update call's own six."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_xarm_amd.device_sac import DeviceSAC  # noqa: E402
from gym_xarm_amd.sac import SacPolicy, make_optimizers, sac_step  # noqa: E402

CALLS = 20
WIDTHS = {"XarmReach-v0": 14, "XarmPDPickAndPlace-v0": 30}
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
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--commit", default=None, help="recorded in the JSON: the commit the figures were taken at")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "steps_per_window": CALLS, "act_dim": ACT_DIM, "legs": []}
    for env_id, D in WIDTHS.items():
        for B in args.batch:
            torch.manual_seed(0)
            model_t = SacPolicy(D, ACT_DIM).cuda()
            model_h = copy.deepcopy(model_t)
            opts = make_optimizers(model_t)
            sac = DeviceSAC(model_h, B)
            batch = {"obs": (torch.rand(B, D, device="cuda") * 2 - 1) * 3, "next_obs": (torch.rand(B, D, device="cuda") * 2 - 1) * 3,
                     "action": torch.rand(B, ACT_DIM, device="cuda") * 2 - 1, "reward": -(torch.rand(B, device="cuda") < 0.8).float(),
                     "done": (torch.rand(B, device="cuda") < 0.04).float(), "use": torch.ones(B, device="cuda")}

            def torch_call():
                sac_step(model_t, opts, batch)

            def hip_call():
                sac.update(batch)

            for _ in range(2):
                torch_call()
                hip_call()
            ms = {}
            for impl, fn in (("torch_first", torch_call), ("hip", hip_call), ("torch_last", torch_call)):
                ms[impl] = timed(fn, CALLS)
                res["legs"].append(dict(widths=env_id, obs_width=D, batch=B, impl=impl, ms_per_step=ms[impl]))
                print(json.dumps(res["legs"][-1]), flush=True)
            res["legs"].append(dict(widths=env_id, obs_width=D, batch=B, impl="ratio", torch_over_hip=min(ms["torch_first"], ms["torch_last"]) / ms["hip"],
                                    spread=abs(ms["torch_last"] - ms["torch_first"]) / ms["torch_first"]))
            print(json.dumps(res["legs"][-1]), flush=True)
            keep = (torch_call, hip_call, sac.launches)
    res["torch_launches"], res["hip_launches"], res["hip_launches_update"] = count_launches(keep[0]), count_launches(keep[1]), keep[2]
    print(json.dumps({k: res[k] for k in ("torch_launches", "hip_launches", "hip_launches_update")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
