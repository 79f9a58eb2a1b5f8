#!/usr/bin/env python3
"""Time xarm_render (k_render) with device events: median of 3 warmed windows per configuration.

  python tools/render_rate.py [--out profiles/render_rate.json] [--images DIR]

Legs: render alone at (4 096 envs, 84 x 84), (16 384, 84 x 84), (65 536, 64 x 64) and (1, 500 x 500) for every env kind;
PickAndPlace step alone against step + render at 4 096 envs, 84 x 84.  Each leg also reports the output bytes of one call
and the ray-primitive tests a call would make without the tile culling (pixels x primitives), the upper bound the culled
count sits under.  --images DIR writes one PNG per env kind (seeded state after 10 random steps, default camera).
Kernel times of their own: rocprofv3 --kernel-trace --stats -- python tools/render_rate.py (profiles/README.md)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gym_xarm_amd  # noqa: E402

KINDS = {"pnp": ("XarmPDPickAndPlace-v0", 4, None, 16), "reach": ("XarmReach-v0", 4, None, 12),
         "handover": ("XarmPDHandover-v0", 8, None, 27), "handover2": ("XarmPDHandover-v0", 8, {"num_obj": 2}, 29),
         "stack": ("XarmPDStackTower-v0", 8, None, 28)}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", default=None)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "render": [], "step_vs_step_render": None}
    for kind, (env_id, A, cfg, nprim) in KINDS.items():
        for E, W, H in ((4096, 84, 84), (16384, 84, 84), (65536, 64, 64), (1, 500, 500)):
            env = gym_xarm_amd.make(env_id, num_envs=E, seed=0, config=cfg)
            env.reset()
            env.step(torch.rand(E, A, device="cuda") * 2 - 1)
            cam = env._camera(None, W, H)
            rgba = torch.empty(E, H, W, 4, device="cuda", dtype=torch.uint8)
            ms = timed(lambda: env.render_into(cam, None, rgba), 20 if E > 1 else 50)
            px = E * W * H
            res["render"].append(dict(kind=kind, envs=E, width=W, height=H, ms=ms, mpix_per_s=px / ms / 1e3, out_bytes=px * 4,
                                      unculled_ray_prim_tests=px * nprim, gbytes_per_s=px * 4 / ms / 1e6))
            print(json.dumps(res["render"][-1]), flush=True)
            env.close()
    E = 4096
    env = gym_xarm_amd.make("XarmPDPickAndPlace-v0", num_envs=E, seed=0)
    env.reset()
    acts = torch.rand(E, 4, device="cuda") * 2 - 1
    cam = env._camera(None, 84, 84)
    rgba = torch.empty(E, 84, 84, 4, device="cuda", dtype=torch.uint8)
    s = timed(lambda: env.step(acts), 20)
    sr = timed(lambda: (env.step(acts), env.render_into(cam, None, rgba)), 20)
    res["step_vs_step_render"] = dict(envs=E, width=84, height=84, step_ms=s, step_render_ms=sr)
    print(json.dumps(res["step_vs_step_render"]), flush=True)
    env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)
    if args.images:
        from PIL import Image
        os.makedirs(args.images, exist_ok=True)
        for kind, (env_id, A, cfg, _) in KINDS.items():
            env = gym_xarm_amd.make(env_id, num_envs=4, seed=11, config=cfg)
            env.reset()
            g = torch.Generator(device="cuda").manual_seed(0)
            for _ in range(10):
                env.step(torch.rand(4, A, device="cuda", generator=g) * 2 - 1)
            img = env.render(camera={"flags": 1})[0].cpu().numpy()
            Image.fromarray(img, "RGBA").save(os.path.join(args.images, "%s.png" % kind))
            env.close()


if __name__ == "__main__":
    main()
