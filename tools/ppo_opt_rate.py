#!/usr/bin/env python3
"""Time DevicePPO.update with the PPO options with device events: the full update, the update with clip_range_vf on,
and an update that target_kl stops at step 1 (step 0 is applied, the other 15 steps are launched and return on the flag), on both
backends - the fused tile at 64-64 tanh and the wide chain at [256, 256, 256] ReLU - at 16 x 4 096 rows of Reach width, 4 epochs x 4
minibatches (S = 16).  The three legs are alternated window by window in one process: `windows` rounds of `iters` calls per leg behind a
warm-up; the median window of each leg and its spread (max - min) / median are recorded.

  python tools/ppo_opt_rate.py [--out profiles/ppo_opt_rate.json] [--key options]

Every leg runs update(shuffle=False) on the same stored rollout and its own copy of the module.  The full and clip legs run at lr = 0
(tools/ppow_rate.py explains why; Adam's work does not depend on lr).  The stopped leg needs a step that moves: lr = 1e-4 and
target_kl = 1e-9, so that step 0 (approx_kl exactly 0) is applied and step 1 trips; the steps applied by the last call are read off stats[:, 7] after
the timing and recorded (1 for the stopped leg, 16 for the others).  --out
merges the result under --key into an existing JSON file."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_xarm_amd.device_ppo import DevicePPO  # noqa: E402
from gym_xarm_amd.train import ActorCritic  # noqa: E402

D, ACT_DIM, N_STEPS, ENVS, N_EPOCHS, MINIBATCHES = 14, 4, 16, 4096, 4, 4
BACKENDS = (("tile64", (64, 64), "tanh"), ("wide", (256, 256, 256), "relu"))
LEGS = (("full", dict(lr=0.0)), ("clip_range_vf", dict(lr=0.0, clip_range_vf=0.2)), ("stopped_at_step_1", dict(lr=1e-4, target_kl=1e-9)))


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def measure(backend, arch, act, iters, windows):
    torch.manual_seed(0)
    n_rows = N_STEPS * ENVS
    model = ActorCritic(D, ACT_DIM, arch, act).cuda()
    obs = (torch.rand(N_STEPS, ENVS, D, device="cuda") * 2 - 1) * 3
    with torch.no_grad():
        action = model.dist(obs).sample()
    reward, done = torch.randn(N_STEPS, ENVS, device="cuda"), (torch.rand(N_STEPS, ENVS, device="cuda") < 0.04).float()
    last = (torch.rand(ENVS, D, device="cuda") * 2 - 1) * 3
    legs = []
    for name, kw in LEGS:
        ppo = DevicePPO(copy.deepcopy(model), ENVS, n_steps=N_STEPS, n_epochs=N_EPOCHS, batch_size=n_rows // MINIBATCHES, **kw)
        assert ppo.backend == backend and ppo.num_steps == 16
        for k, t in (("obs", obs), ("action", action), ("reward", reward), ("done", done)):
            ppo.buffers[k].copy_(t)
        ppo.shuffle()
        legs.append((name, ppo, (lambda p=ppo: p.update(last, shuffle=False))))
    for _, _, fn in legs:
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in legs}
    for _ in range(windows):
        for name, _, fn in legs:
            times[name].append(window(fn, iters))
    out = []
    for name, ppo, _ in legs:
        t = sorted(times[name])
        med = t[len(t) // 2]
        applied = ppo.steps_applied()
        out.append(dict(backend=backend, net_arch=list(arch), activation=act, rows=n_rows, steps=16, leg=name, steps_applied=applied, launches=ppo.launches,
                        ms_per_update=med, spread=(t[-1] - t[0]) / med))
        print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--key", default="options")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "obs_width": D, "act_dim": ACT_DIM, "n_steps": N_STEPS, "num_envs": ENVS, "n_epochs": N_EPOCHS,
           "minibatches": MINIBATCHES, "iters": args.iters, "windows": args.windows, "legs": []}
    for backend, arch, act in BACKENDS:
        res["legs"] += measure(backend, arch, act, args.iters, args.windows)
    if args.out:
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc[args.key] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
