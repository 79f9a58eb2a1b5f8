#!/usr/bin/env python3
"""Time policy evaluation (gym_xarm_amd/evaluation.py): the accounting alone and whole evaluations.

  python tools/eval_rate.py [--out profiles/eval_rate.json] [--sizes reach:4096 pnp:65536]

Two sizes: XarmReach-v0 at 4 096 envs with N = 4 096 and XarmPDPickAndPlace-v0 at 65 536 envs with N = 65 536, an untrained seeded 64-64
ActorCritic through DevicePolicy, deterministic, under a DeviceVecNormalize's frozen statistics.  One process; per size, after a warm-up
of every leg, three rounds that alternate the legs.

accounting: a synthetic stream (random float32 rewards; env e finishes when (e + t) % 50 == 0; uint8 done and success as the VecEnv
hands them out), no env step.  `hip` is DeviceEvaluator.step_into - one launch, nothing read back; `torch` is the checker's per-step
accounting (evaluation.TorchAccounting.step: about a dozen launches and the host read of SB3's loop condition).  A window is 50 steps
timed with device events (the torch leg's host reads fall inside its window); ms per step.
evaluation: whole runs, wall clock around a device synchronisation, in ms, with the env steps each took: DeviceEvaluator.run eager,
DeviceEvaluator.run graph=True (the capture is made in the warm-up and reused) and evaluate_policy_torch."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_xarm_amd  # noqa: E402
from gym_xarm_amd import evaluation as EV  # noqa: E402
from gym_xarm_amd.device_policy import DevicePolicy  # noqa: E402
from gym_xarm_amd.normalize import DeviceVecNormalize  # noqa: E402
from gym_xarm_amd.train import ActorCritic  # noqa: E402

ENVS = {"reach": "XarmReach-v0", "pnp": "XarmPDPickAndPlace-v0"}
EP_LEN, ROUNDS = 50, 3


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def accounting_legs(res, name, E, N):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    rew = [torch.rand(E, device=dev, generator=g) for _ in range(EP_LEN)]
    e = torch.arange(E, device=dev)
    done = [((e + t) % EP_LEN == 0).to(torch.uint8) for t in range(EP_LEN)]
    succ = [((e + 3 * t) % 7 == 0).to(torch.uint8) for t in range(EP_LEN)]
    ev = EV.DeviceEvaluator(type("W", (), dict(num_envs=E, device=dev))(), N)
    ev.begin()
    acc = EV.TorchAccounting(E, N, dev)
    pos = {"hip": 0, "torch": 0}

    def hip():
        k = pos["hip"] % EP_LEN
        ev.step_into(rew[k], done[k], succ[k])
        pos["hip"] += 1

    def torch_():
        k = pos["torch"] % EP_LEN
        acc.step(rew[k], done[k], succ[k])
        pos["torch"] += 1
    legs = (("hip", hip), ("torch", torch_))
    for _, fn in legs:
        window(fn, EP_LEN)
    for rnd in range(ROUNDS):
        for impl, fn in legs:
            rec = dict(size=name, envs=E, episodes=N, leg="accounting", impl=impl, round=rnd, ms_per_step=window(fn, EP_LEN))
            res["legs"].append(rec)
            print(json.dumps(rec), flush=True)
    torch.cuda.synchronize()
    assert bool(torch.equal(ev.records, acc.records))       # the two were fed the same stream
    del ev, acc
    torch.cuda.empty_cache()


def evaluation_legs(res, name, E, N):
    envs = [gym_xarm_amd.make(ENVS[name], num_envs=E, seed=1) for _ in range(3)]
    venv = DeviceVecNormalize(envs[0], monitor_capacity=max(E, 1))
    venv.stats[:venv.dim] = 0.25
    torch.manual_seed(0)
    model = ActorCritic(venv.dim, envs[0].act_dim).cuda()
    policy = EV.as_policy(DevicePolicy(model, seed=0), venv)
    eager, graphed = EV.DeviceEvaluator(envs[0], N), EV.DeviceEvaluator(envs[1], N)
    legs = (("eager", lambda: eager.run(policy)), ("graph", lambda: graphed.run(policy, graph=True)),
            ("torch", lambda: EV.evaluate_policy_torch(policy, envs[2], N, full=True)[0]))
    for _, fn in legs:
        fn()
    for rnd in range(ROUNDS):
        for impl, fn in legs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            rec = dict(size=name, envs=E, episodes=N, leg="evaluation", impl=impl, round=rnd, ms=ms, steps=out["steps"], ms_per_step=ms / out["steps"],
                       mean_reward=out["mean_reward"], success_rate=out["success_rate"])
            res["legs"].append(rec)
            print(json.dumps(rec), flush=True)
    for env in envs:
        env.close()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", nargs="+", default=["reach:4096", "pnp:65536"])
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "episode_length": EP_LEN, "rounds": ROUNDS, "legs": [], "acceptance": []}
    for size in args.sizes:
        name, E = size.split(":")
        accounting_legs(res, name, int(E), int(E))
        evaluation_legs(res, name, int(E), int(E))
        hip = [x["ms_per_step"] for x in res["legs"] if x["size"] == name and x["leg"] == "accounting" and x["impl"] == "hip"]
        tor = [x["ms_per_step"] for x in res["legs"] if x["size"] == name and x["leg"] == "accounting" and x["impl"] == "torch"]
        res["acceptance"].append(dict(size=name, hip_max_ms=max(hip), torch_min_ms=min(tor), every_hip_window_below_every_torch_window=max(hip) < min(tor)))
        print(json.dumps(res["acceptance"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
