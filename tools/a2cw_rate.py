#!/usr/bin/env python3
"""Time the wide A2C device update with device events: train.py's a2c_update on ActorCritic(net_arch, activation) against
device_a2c.py's DeviceA2C.update on its "wide" backend (3 L + 7 HIP launches).  Median of 3 warmed windows per leg; the torch leg runs
first and again last (drift), `spread` is (max - min) / median of a leg's windows.

  python tools/a2cw_rate.py [--out profiles/a2cw_rate.json] [--envs 256 4096 65536] [--learn] [--no-rate] [--commit ID]

Shapes [256, 256, 256] ReLU and [256, 256] tanh, Reach widths (14 columns) and PickAndPlace widths (30), act_dim 4; n_steps 5 at 256, 4 096
and 65 536 envs.  Both legs read the same stored rollout and start from the same module; each updates its own copy, with lr = 0 in both
optimisers: a leg repeats its update on one rollout dozens of times, and with a real learning rate (RMSprop's first steps move every entry
by about 10 lr) the wide module leaves the region the update is meant for; RMSprop's work per step does not depend on lr.  The kernels per
update are counted with the torch profiler after the last timed window (a tracer slows the host: nothing is timed once it has been
started) and compared with DeviceA2C.launches.  --learn: dense Reach with [256, 256] tanh and A2C's defaults, the torch block and the
device path at the same sizes and seed - the record tests/test_a2cw_gpu.py::test_wide_device_a2c_learns_reach reads."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_xarm_amd.device_a2c import DeviceA2C  # noqa: E402
from gym_xarm_amd.train import ActorCritic, a2c_update, train  # noqa: E402

WIDTHS = {"XarmReach-v0": 14, "XarmPDPickAndPlace-v0": 30}
SHAPES = (((256, 256, 256), "relu"), ((256, 256), "tanh"))
ACT_DIM, N_STEPS, GAMMA = 4, 5, 0.99
LEARN = dict(num_envs=2048, updates=300)


def timed(fn, iters, windows=3):
    """(median ms per call, spread) over `windows` windows of `iters` calls behind one warm-up call"""
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
    med = sorted(out)[len(out) // 2]
    return med, (max(out) - min(out)) / med


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


def update_legs(res, env_id, D, arch, act, E):
    torch.manual_seed(0)
    model_t = ActorCritic(D, ACT_DIM, arch, act).cuda()
    model_h = copy.deepcopy(model_t)
    opt = torch.optim.RMSprop(model_t.parameters(), lr=0.0, alpha=0.99, eps=1e-5)
    a2c = DeviceA2C(model_h, E, n_steps=N_STEPS, gamma=GAMMA, lr=0.0, wide=True)
    assert a2c.backend == "wide"
    b = a2c.buffers
    b["obs"].copy_((torch.rand(N_STEPS, E, D, device="cuda") * 2 - 1) * 3)
    with torch.no_grad():
        b["action"].copy_(model_t.dist(b["obs"]).sample())
    b["reward"].normal_()
    b["done"].copy_((torch.rand(N_STEPS, E, device="cuda") < 0.04).float())
    last = (torch.rand(E, D, device="cuda") * 2 - 1) * 3
    rollout = {k: b[k].clone() for k in ("obs", "action", "reward", "done", "use")}

    def torch_call():
        a2c_update(model_t, opt, rollout, last, GAMMA)

    def hip_call():
        a2c.update(last)

    iters = 20 if E <= 4096 else 5
    for _ in range(2):
        torch_call()
        hip_call()
    for impl, fn in (("torch_first", torch_call), ("hip", hip_call), ("torch_last", torch_call)):
        ms, spread = timed(fn, iters)
        res["update"].append(dict(widths=env_id, obs_width=D, net_arch=list(arch), activation=act, num_envs=E, rows=N_STEPS * E, impl=impl,
                                  ms_per_update=ms, spread=spread, workspace_bytes=int(b["workspace"].numel()) * 4))
        print(json.dumps(res["update"][-1]), flush=True)
    return torch_call, hip_call, a2c.launches


def learn(res):
    """dense Reach, [256, 256] tanh, A2C's defaults: the torch block, then the device path, at the same sizes and seed"""
    rec = dict(LEARN, net_arch=[256, 256], activation="tanh", env="XarmReach-v0", reward_type="dense")
    for name, flags in (("torch", dict()), ("hip", dict(device_update=True, device_policy=True, device_normalize=True, wide=True))):
        model, venv, hist = train("XarmReach-v0", num_envs=LEARN["num_envs"], updates=LEARN["updates"], algo="a2c", net_arch=(256, 256), activation="tanh",
                                  config={"reward_type": "dense", "GUI": False}, log_every=LEARN["updates"] // 2, quiet=True, **flags)
        rec[name] = dict(first=hist[0]["mean_raw_reward"], last=hist[-1]["mean_raw_reward"], success_first=hist[0]["success_rate"],
                         success_last=hist[-1]["success_rate"], env_steps_per_sec=hist[-1]["env_steps_per_sec"])
        print(json.dumps({name: rec[name]}), flush=True)
    res["learn"] = rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, nargs="+", default=[256, 4096, 65536])
    ap.add_argument("--learn", action="store_true")
    ap.add_argument("--no-rate", action="store_true", help="with --learn: the learning runs only")
    ap.add_argument("--commit", default=None, help="recorded in the JSON: the commit the figures were taken at")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "commit": args.commit, "n_steps": N_STEPS, "act_dim": ACT_DIM, "update": []}
    if args.out and os.path.exists(args.out):                  # a later run keeps what it does not retake
        old = json.load(open(args.out))
        res.update({k: old[k] for k in ("update", "learn", "launches") if k in old and (args.no_rate or k == "learn")})
    if not args.no_rate:
        res["update"], counted = [], []
        for env_id, D in WIDTHS.items():
            for arch, act in SHAPES:
                for E in args.envs:
                    legs = update_legs(res, env_id, D, arch, act, E)
                    if D == 14 and E == args.envs[0]:              # counted behind the last timed window, at the smallest size
                        counted.append((arch, act, E, legs))
        res["launches"] = [dict(net_arch=list(arch), activation=act, num_envs=E, torch=count_launches(legs[0]), hip=count_launches(legs[1]), hip_update=legs[2])
                           for arch, act, E, legs in counted]
        print(json.dumps(res["launches"]), flush=True)
    if args.learn:
        learn(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
