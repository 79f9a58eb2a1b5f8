#!/usr/bin/env python3
"""Time xarm_render_views (k_render_views) against xarm_render (k_render) with device events: median of 3 warmed windows.

  python tools/render_views_rate.py [--out profiles/render_views_rate.json] [--envs 4096] [--size 84]

Legs, PickAndPlace after one random step: (a) xarm_render with the default camera - the yardstick; (b) xarm_render_views with
that camera converted to one world view; (c) {world, wrist0} in one V = 2 call against the two single-view calls, and the
wrist view alone; (d) the V = 2 call with per-env records ([n, V, 16], identical rows) against the shared [V, 16] records."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gym_xarm_amd  # noqa: E402
from render_rate import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--size", type=int, default=84)
    args = ap.parse_args()
    E, S = args.envs, args.size
    env = gym_xarm_amd.make("XarmPDPickAndPlace-v0", num_envs=E, seed=0)
    env.reset()
    env.step(torch.rand(E, 4, device="cuda") * 2 - 1)
    cam = env._camera(None, S, S)
    dv = env.default_views()
    world, wrist, both = dv["world"][None].contiguous(), dv["wrist0"][None].contiguous(), torch.stack([dv["world"], dv["wrist0"]])
    per = both[None].repeat(E, 1, 1).contiguous()
    r1 = torch.empty(E, 1, S, S, 4, device="cuda", dtype=torch.uint8)
    r2 = torch.empty(E, 2, S, S, 4, device="cuda", dtype=torch.uint8)
    it = 20
    res = {"device": torch.cuda.get_device_name(0), "kind": "pnp", "envs": E, "width": S, "height": S, "iters": it, "windows": 3}
    res["a_render_ms"] = timed(lambda: env.render_into(cam, None, r1), it)
    res["b_views_world_ms"] = timed(lambda: env.render_views_into(world, 0, S, S, 0, None, r1), it)
    res["c_views_wrist_ms"] = timed(lambda: env.render_views_into(wrist, 0, S, S, 0, None, r1), it)
    res["c_views_world_wrist_one_call_ms"] = timed(lambda: env.render_views_into(both, 0, S, S, 0, None, r2), it)
    res["c_views_world_wrist_two_calls_ms"] = timed(lambda: (env.render_views_into(world, 0, S, S, 0, None, r1),
                                                              env.render_views_into(wrist, 0, S, S, 0, None, r1)), it)
    res["d_views_world_wrist_per_env_ms"] = timed(lambda: env.render_views_into(per, 1, S, S, 0, None, r2), it)
    res["a_again_render_ms"] = timed(lambda: env.render_into(cam, None, r1), it)
    res["b_over_a"] = res["b_views_world_ms"] / res["a_render_ms"]
    print(json.dumps(res), flush=True)
    env.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
