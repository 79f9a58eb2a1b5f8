"""The device-resident VecNormalize + monitor on the MI355X (gym_xarm_amd/normalize.py DeviceVecNormalize, csrc/xarm_k_norm.hip):
the kernels against the host build of the same core bit for bit at the wavefront and chunk edges, one large batch, determinism,
a captured step_into against eager calls, a live env against the torch classes, and the training driver on the device class."""
import json
import os

import numpy as np
import pytest
import torch

import norm_host as NH
from gym_xarm_amd.normalize import DeviceVecNormalize
from gym_xarm_amd.train import EpisodeMonitor, VecNormalize

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 127, 128, 129, 1000)
STATE = ("stats", "ret", "ep_ret", "ep_len", "ring", "n")


class Label:
    """what DeviceVecNormalize is told about its env: sizes and device"""

    def __init__(self, E, od, gd):
        self.num_envs, self.obs_dim, self.goal_dim, self.act_dim, self.device = E, od, gd, 1, torch.device("cuda")
        self.flat_observation = gd == 0


def dev_state(dv):
    m = dv.monitor
    return {"stats": dv.stats, "ret": dv.ret, "ep_ret": m.ep_ret, "ep_len": m.ep_len, "ring": m.ring, "n": m.n_dev}


def to_dev(parts):
    t = [None if p is None else torch.from_numpy(p).cuda() for p in parts]
    return t[0] if t[1] is None else {"observation": t[0], "achieved_goal": t[1], "desired_goal": t[2]}


def device_step(dv, out, s, t, t_seconds):
    """one poisoned step_into of stream call t"""
    dv.work.view(torch.uint8).fill_(0xFF)
    out["nobs"].fill_(float("nan"))
    out["nrew"].fill_(float("nan"))
    keep = None if s.keep[t] is None else torch.from_numpy(s.keep[t]).cuda()
    dv.step_into(out, to_dev(s.parts(t)), torch.from_numpy(s.rew[t]).cuda(), torch.from_numpy(s.done[t]).cuda(), keep, t_seconds=t_seconds)


def assert_same_state(dv, host, what):
    for k, v in dev_state(dv).items():
        assert NH.bits(v.cpu().numpy()) == NH.bits(getattr(host, k)), (what, k)


@pytest.mark.parametrize("od,gd", NH.WIDTHS)
@pytest.mark.parametrize("E", SIZES)
def test_kernels_equal_the_host_build_bit_for_bit(E, od, gd):
    """twelve consecutive calls per (keep, done) case; outputs and workspace are NaN / 0xFF before every call on both sides"""
    for keep_mode in ("none", "mixed", "dropped"):
        for done_mode in ("none", "all", "edge"):
            s = NH.Stream(E, od, gd, calls=12, seed=3, done_mode=done_mode, keep_mode=keep_mode)
            cap = max(E, 8) + 3                                       # wraps under 'all', at a row that is no chunk edge
            dv, host = DeviceVecNormalize(Label(E, od, gd), monitor_capacity=cap), NH.HostNorm(E, od, gd, capacity=cap)
            env = NH.StreamEnv(s, "cuda")
            dv.env = env
            dv.work.view(torch.uint8).fill_(0xFF)
            case = (keep_mode, done_mode)
            assert NH.bits(dv.reset().cpu().numpy()) == NH.bits(host.reset(s.parts())), case
            assert_same_state(dv, host, case)
            out = dv.alloc_out()
            for t in range(s.calls):
                device_step(dv, out, s, t, 0.25 * t)
                h_obs, h_rew = host.step(s.parts(t), s.rew[t], s.done[t], s.keep[t], t=0.25 * t)
                assert NH.bits(out["nobs"].cpu().numpy()) == NH.bits(h_obs), (case, t)
                assert NH.bits(out["nrew"].cpu().numpy()) == NH.bits(h_rew), (case, t)
                assert_same_state(dv, host, (case, t))
            fins = int(sum(int(d.sum()) for d in s.done))
            assert int(dv.monitor.n) == fins == {"none": 0, "all": 12 * E, "edge": 12 * min(E, 2 if E > 128 else 1)}[done_mode]
            if keep_mode == "dropped":
                assert NH.bits(dv.stats[2 * s.D:].cpu().numpy()) == NH.bits(np.array([0.0, 1.0, 1e-4 + E, 1e-4]))   # the reset's rows only
    # training off: the statistics stay, the monitor goes on
    dv.training = host.training = False
    before = dv.stats.clone()
    device_step(dv, out, s, 0, 9.0)
    h_obs, h_rew = host.step(s.parts(0), s.rew[0], s.done[0], s.keep[0], t=9.0)
    assert NH.bits(out["nobs"].cpu().numpy()) == NH.bits(h_obs) and NH.bits(out["nrew"].cpu().numpy()) == NH.bits(h_rew)
    assert torch.equal(dv.stats, before)
    assert_same_state(dv, host, "training off")


def test_one_large_batch_equals_the_host_build():
    E, od, gd = 65536, 24, 3
    s = NH.Stream(E, od, gd, calls=1, seed=5)
    s.done[0] = (np.arange(E) % 50 == 7).astype(np.uint8)
    s.keep[0] = (np.arange(E) % 11 != 0).astype(np.uint8)
    dv, host = DeviceVecNormalize(Label(E, od, gd), monitor_capacity=E), NH.HostNorm(E, od, gd, capacity=E)
    out = dv.alloc_out()
    device_step(dv, out, s, 0, 1.0)
    h_obs, h_rew = host.step(s.parts(0), s.rew[0], s.done[0], s.keep[0], t=1.0)
    assert NH.bits(out["nobs"].cpu().numpy()) == NH.bits(h_obs) and NH.bits(out["nrew"].cpu().numpy()) == NH.bits(h_rew)
    assert_same_state(dv, host, "large")
    assert int(dv.monitor.n) == int(s.done[0].sum()) == 1311


def test_same_inputs_twice_give_the_same_bits():
    E, od, gd = 1000, 68, 12
    s = NH.Stream(E, od, gd, calls=4, seed=9, keep_mode="mixed")
    runs = []
    for _ in range(2):
        dv = DeviceVecNormalize(Label(E, od, gd), monitor_capacity=E)
        out, outs = dv.alloc_out(), []
        for t in range(s.calls):
            device_step(dv, out, s, t, 2.0)
            outs.append((out["nobs"].clone(), out["nrew"].clone()))
        runs.append((outs, {k: v.clone() for k, v in dev_state(dv).items()}))
    (a_out, a_state), (b_out, b_state) = runs
    for (ao, ar), (bo, br) in zip(a_out, b_out):
        assert NH.bits(ao.cpu().numpy()) == NH.bits(bo.cpu().numpy()) and NH.bits(ar.cpu().numpy()) == NH.bits(br.cpu().numpy())
    for k in STATE:
        assert NH.bits(a_state[k].cpu().numpy()) == NH.bits(b_state[k].cpu().numpy()), k
    assert float(a_state["stats"][2 * s.D + 2]) > 1000.0


def test_captured_step_into_replays_like_eager_calls():
    E, od, gd = 1000, 24, 3
    s = NH.Stream(E, od, gd, calls=7, seed=2)
    cap, twin = (DeviceVecNormalize(Label(E, od, gd), monitor_capacity=2048) for _ in range(2))
    obs = to_dev(s.parts(0))
    rew, done = torch.from_numpy(s.rew[0]).cuda(), torch.from_numpy(s.done[0]).cuda()
    keep = torch.ones(E, device="cuda", dtype=torch.uint8)
    out, ref = cap.alloc_out(), twin.alloc_out()

    def load(t):                                                       # the static inputs, rewritten in place
        for k, p in zip(("observation", "achieved_goal", "desired_goal"), s.parts(t)):
            obs[k].copy_(torch.from_numpy(p))
        rew.copy_(torch.from_numpy(s.rew[t]))
        done.copy_(torch.from_numpy(s.done[t]))
        keep.copy_(torch.from_numpy(s.keep[t] if s.keep[t] is not None else np.ones(E, np.uint8)))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cap.step_into(out, obs, rew, done, keep, t_seconds=1.5)      # warm-up call on stream call 0
    torch.cuda.current_stream().wait_stream(side)
    twin.step_into(ref, obs, rew, done, keep, t_seconds=1.5)
    graph = torch.cuda.CUDAGraph()
    load(1)
    with torch.cuda.graph(graph):
        cap.step_into(out, obs, rew, done, keep, t_seconds=1.5)      # no allocation, no host read: it captures (nothing runs yet)
    counts, ns = [float(cap.stats[2 * s.D + 2])], [int(cap.monitor.n)]
    for t in range(1, 6):
        load(t)
        graph.replay()
        twin.step_into(ref, obs, rew, done, keep, t_seconds=1.5)
        torch.cuda.synchronize()
        assert torch.equal(out["nobs"], ref["nobs"]) and torch.equal(out["nrew"], ref["nrew"]), t
        for (k, a), b in zip(dev_state(cap).items(), dev_state(twin).values()):
            assert NH.bits(a.cpu().numpy()) == NH.bits(b.cpu().numpy()), (t, k)
        counts.append(float(cap.stats[2 * s.D + 2]))
        ns.append(int(cap.monitor.n))
    kept = [E if s.keep[t] is None else int(s.keep[t].sum()) for t in range(1, 6)]
    assert np.array_equal(np.round(np.diff(counts), 6), kept)         # every replay merged its own batch
    assert np.array_equal(np.diff(ns), [int(s.done[t].sum()) for t in range(1, 6)]) and min(np.diff(ns)) > 0


def test_live_env_against_the_torch_classes():
    """XarmReach-v0, 256 envs, 60 steps on twin envs: the wrapper writes nothing the env owns, the normalised outputs agree
    with the torch classes within twice their own deviation from the float64 restatement on this stream plus a float32 ulp,
    and the monitors hold the same 2 x 256 rows"""
    import gym_xarm_amd
    E, steps = 256, 60
    ea, eb = (gym_xarm_amd.make("XarmReach-v0", num_envs=E, seed=4) for _ in range(2))
    tv, tm = VecNormalize(ea), EpisodeMonitor(E, ea.device, capacity=1024)
    dv = DeviceVecNormalize(eb, monitor_capacity=1024)
    D = dv.dim
    ref = NH.Ref64(E, D, 1024)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    cat = lambda o: torch.cat([o["observation"], o["achieved_goal"], o["desired_goal"]], 1).cpu().numpy()

    def torch_stats():
        return np.concatenate([tv.obs_rms.mean.cpu().numpy().astype(np.float64), tv.obs_rms.var.cpu().numpy().astype(np.float64),
                               [float(tv.ret_rms.mean), float(tv.ret_rms.var)]])

    t_obs, d_obs = tv.reset(), dv.reset()
    assert torch.equal(ea.get_state(), eb.get_state())
    rows = cat({"observation": ea._obs, "achieved_goal": ea._ag, "desired_goal": ea._dg})
    trace = [(t_obs.cpu().numpy(), None, torch_stats(), d_obs.cpu().numpy(), None, dv.stats[:2 * D + 2].cpu().numpy(), ref.reset(rows), None, ref.stats()[:2 * D + 2])]
    for k in range(steps):
        a = torch.rand(E, ea.act_dim, device="cuda", generator=g) * 2 - 1
        t_obs, t_rew, t_done, t_info, t_raw = tv.step(a)
        tm.update(t_raw, t_done)
        d_obs, d_rew, d_done, d_info, d_raw = dv.step(a)
        assert torch.equal(t_raw, d_raw) and torch.equal(t_done, d_done), k
        for key in ("_obs", "_ag", "_dg"):
            assert torch.equal(getattr(ea, key), getattr(eb, key)), (k, key)
        rows = cat({"observation": eb._obs, "achieved_goal": eb._ag, "desired_goal": eb._dg})
        r_obs, r_rew = ref.step(rows, d_raw.cpu().numpy(), d_done.cpu().numpy())
        trace.append((t_obs.cpu().numpy(), t_rew.cpu().numpy(), torch_stats(), d_obs.cpu().numpy(), d_rew.cpu().numpy(),
                      dv.stats[:2 * D + 2].cpu().numpy(), r_obs, r_rew, ref.stats()[:2 * D + 2]))
    assert torch.equal(ea.get_state(), eb.get_state())
    dev, mag = [0.0] * 3, [0.0] * 3
    for row in trace:
        for q in range(3):
            if row[q] is not None:
                dev[q] = max(dev[q], float(np.abs(row[q].astype(np.float64) - row[6 + q]).max()))
                mag[q] = max(mag[q], float(np.abs(row[6 + q]).max()))
    tol = [2.0 * dev[q] + float(NH.ulp32(mag[q])) for q in range(3)]
    worst = [0.0] * 3
    for row in trace:
        for q in range(3):
            if row[q] is not None:
                worst[q] = max(worst[q], float(np.abs(row[3 + q].astype(np.float64) - row[q]).max()))
    print("live Reach 256 x 60 (nobs, nrew, stats): torch - float64 %s, tolerance %s, device - torch %s" % (dev, tol, worst))
    for q in range(3):
        assert worst[q] <= tol[q], (q, worst, tol)
    assert int(dv.monitor.n) == 2 * E == tm.n
    assert float(dv.stats[2 * D + 2]) == tv.obs_rms.count and float(dv.stats[2 * D + 3]) == tv.ret_rms.count
    assert torch.equal(dv.monitor.ring[:2 * E, :2], tm.ring[:2 * E, :2])
    assert torch.equal(dv.monitor.ep_ret, tm.ep_ret) and torch.equal(dv.monitor.ep_len, tm.ep_len)
    r, l = dv.monitor.last(100)
    assert r.shape == (100,) and bool((l == 25).all()) and dv.monitor.mean_reward(2 * E) == pytest.approx(float(tm.ring[:2 * E, 0].mean()))
    ea.close()
    eb.close()


def test_driver_on_the_device_class(tmp_path):
    from gym_xarm_amd.train import train
    log_dir = str(tmp_path / "run")
    model, venv, hist = train(env_id="XarmReach-v0", num_envs=256, updates=10, device_normalize=True, log_dir=log_dir, quiet=True,
                              check_freq=20)
    assert isinstance(venv, DeviceVecNormalize) and len(hist) == 1 and hist[0]["episodes"] == 512
    lines = open(os.path.join(log_dir, "0.monitor.csv")).read().splitlines()
    head = json.loads(lines[0][1:])
    assert lines[0].startswith("#") and head["env_id"] == "XarmReach-v0" and "t_start" in head and lines[1] == "r,l,t"
    assert len(lines) == 2 + 512 == 2 + venv.monitor.n
    t_prev = 0.0
    for ln in lines[2:]:
        r, l, t = ln.split(",")
        assert int(l) == 25 and float(t) >= t_prev
        t_prev = float(t)
    assert venv.callback.saves >= 1 and os.path.exists(os.path.join(log_dir, "best_model.safetensors"))

    class Sizes:
        device, num_envs, obs_dim, goal_dim = torch.device("cpu"), 256, 8, 3
    tv = VecNormalize.load(os.path.join(log_dir, "vec_normalize.safetensors"), Sizes())
    assert torch.equal(tv.obs_rms.mean, venv.obs_mean.float().cpu()) and torch.equal(tv.obs_rms.var, venv.obs_var.float().cpu())
    assert tv.obs_rms.count == pytest.approx(1e-4 + 256 * 51, abs=1e-9) and tv.ret_rms.count == pytest.approx(1e-4 + 256 * 50, abs=1e-9)
