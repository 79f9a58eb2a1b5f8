#!/usr/bin/env python3
"""Time the PPO update with device events: train.py's ppo_update - values and old log-probabilities, the GAE loop, and per
minibatch the forward under autograd, the normalised clipped surrogate, backward, clip_grad_norm_ and Adam.step - against
device_ppo.py's DevicePPO.update (4 + 3 S HIP launches).  Median of 3 warmed windows of 10 updates per leg.

  python tools/ppo_rate.py [--out profiles/ppo_rate.json] [--envs 4096 65536] [--commit ID]

n_steps 16 at 4 096 and 65 536 envs (16 x 4 096 and 16 x 65 536 rows), 4 epochs x 4 minibatches (S = 16 optimiser steps per update),
Reach widths (14 columns) and PickAndPlace widths (30), act_dim 4.  Both legs read the same stored rollout and start from the same
ActorCritic; each updates its own copy and draws its own permutations (torch.randperm per epoch in both).  Legs per size and width, in
this order: torch, hip, torch again (drift).  `torch_launches` is the number of kernels the torch leg enqueues per update, counted
with the torch profiler after the last timed window of the run (a tracer slows the host: nothing is timed once it has been
started); `hip_launches` is counted the same way and `hip_launches_update` is the update call's own 4 + 3 S (the rest is the
shuffle)."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_xarm_amd.device_ppo import DevicePPO  # noqa: E402
from gym_xarm_amd.train import ActorCritic, ppo_update  # noqa: E402

CALLS = 10
WIDTHS = {"XarmReach-v0": 14, "XarmPDPickAndPlace-v0": 30}
ACT_DIM, N_STEPS, N_EPOCHS, MINIBATCHES, GAMMA, LAMBDA, CLIP = 4, 16, 4, 4, 0.99, 0.95, 0.2


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
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--commit", default=None, help="recorded in the JSON: the commit the figures were taken at")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "updates_per_window": CALLS, "n_steps": N_STEPS, "n_epochs": N_EPOCHS,
           "minibatches": MINIBATCHES, "act_dim": ACT_DIM, "legs": []}
    for env_id, D in WIDTHS.items():
        for E in args.envs:
            torch.manual_seed(0)
            n_rows = N_STEPS * E
            batch_size = -(-n_rows // MINIBATCHES)
            model_t = ActorCritic(D, ACT_DIM).cuda()
            model_h = copy.deepcopy(model_t)
            opt = torch.optim.Adam(model_t.parameters(), lr=3e-4, eps=1e-5)
            ppo = DevicePPO(model_h, E, n_steps=N_STEPS, n_epochs=N_EPOCHS, batch_size=batch_size, gamma=GAMMA, gae_lambda=LAMBDA, clip_range=CLIP)
            b = ppo.buffers
            b["obs"].copy_((torch.rand(N_STEPS, E, D, device="cuda") * 2 - 1) * 3)
            with torch.no_grad():
                b["action"].copy_(model_t.dist(b["obs"]).sample())
            b["reward"].normal_()
            b["done"].copy_((torch.rand(N_STEPS, E, device="cuda") < 0.04).float())
            last = (torch.rand(E, D, device="cuda") * 2 - 1) * 3
            rollout = {k: b[k].clone() for k in ("obs", "action", "reward", "done", "use")}

            def torch_call():
                # what train(algo="ppo") runs per update without device_update
                ppo_update(model_t, opt, rollout, last, N_EPOCHS, batch_size, GAMMA, LAMBDA, CLIP)

            def hip_call():
                ppo.update(last)

            for _ in range(2):
                torch_call()
                hip_call()
            for impl, fn in (("torch_first", torch_call), ("hip", hip_call), ("torch_last", torch_call)):
                ms = timed(fn, CALLS)
                res["legs"].append(dict(widths=env_id, obs_width=D, num_envs=E, rows=n_rows, steps=ppo.num_steps, impl=impl, ms_per_update=ms))
                print(json.dumps(res["legs"][-1]), flush=True)
            keep = (torch_call, hip_call, ppo.launches)
    res["torch_launches"], res["hip_launches"], res["hip_launches_update"] = count_launches(keep[0]), count_launches(keep[1]), keep[2]
    print(json.dumps({k: res[k] for k in ("torch_launches", "hip_launches", "hip_launches_update")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
