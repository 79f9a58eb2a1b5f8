#!/usr/bin/env python3
"""XarmRearrange-v0 throughput: N envs (default 8 192, StackTower's per-GPU size), uniform random actions, auto-reset on.
Prints env steps/s and ms per step() call, and the row-set class histogram (csrc/xarm_stack_core.h with N = 4: bits 0-5 cube pairs
01 02 03 12 13 23, bit 6 / 7 a pad of arm 0 / 1) after reset() and after the timed steps.  --class-order 0 builds the handle
with XARM_RA_CLASS_ORDER=0 (the plain visiting order).  --json FILE also writes the numbers.  bench.py is not involved."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def class_table(keys):
    import torch
    k = keys.to(torch.int64)
    pairs = torch.zeros_like(k)
    for b in range(6):
        pairs += (k >> b) & 1
    n = float(k.numel())
    return {"no_contact": float((k == 0).sum()) / n,
            "pair_any": float((pairs > 0).sum()) / n,
            "pairs_ge2": float((pairs >= 2).sum()) / n,
            "pairs_ge3": float((pairs >= 3).sum()) / n,
            "pad_arm0": float(((k >> 6) & 1).sum()) / n,
            "pad_arm1": float(((k >> 7) & 1).sum()) / n,
            "classes_present": int(torch.unique(k).numel())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--class-order", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not a.class_order:
        os.environ["XARM_RA_CLASS_ORDER"] = "0"
    import torch
    import gym_xarm_amd
    env = gym_xarm_amd.make("XarmRearrange-v0", num_envs=a.envs, seed=a.seed)
    env.reset()
    torch.cuda.synchronize()
    out = {"envs": a.envs, "steps": a.steps, "class_order": bool(a.class_order)}
    if a.class_order:
        out["classes_after_reset"] = class_table(env.class_keys())
    gen = torch.Generator(device=env.device)
    gen.manual_seed(a.seed)
    acts = [torch.rand(a.envs, 8, device=env.device, generator=gen) * 2 - 1 for _ in range(8)]
    for k in range(a.warmup):
        env.step(acts[k % 8])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(a.steps):
        env.step(acts[k % 8])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out["ms_per_call"] = 1e3 * dt / a.steps
    out["env_steps_per_s"] = a.envs * a.steps / dt
    if a.class_order:
        out["classes_after_steps"] = class_table(env.class_keys())
    out["library"] = env.library()[0]
    env.close()
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
