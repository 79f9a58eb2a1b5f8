"""The device-resident VecNormalize + monitor's core (gym_xarm_amd/csrc/xarm_norm_core.h) on the CPU: the g++ build
(tests/norm_host.py) against a float64 NumPy restatement of train.py's classes and against the torch classes themselves on one
scripted stream, the statistics that must not move, state interchange between DeviceVecNormalize and VecNormalize, the argument
checks of the three C-ABI entry points through the real library (no device needed), and an address / undefined-behaviour
sanitizer run of the host core as a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import norm_host as NH
from gym_xarm_amd.train import EpisodeMonitor, VecNormalize

SIZES = (1, 127, 128, 129, 1000)
_runs = {}


def run(E, od, gd):
    """the 30-call stream through the host core, the float64 restatement and the torch classes; every call's outputs and the
    statistics after it are kept.  Computed once per case and only read."""
    key = (E, od, gd)
    if key in _runs:
        return _runs[key]
    s = NH.Stream(E, od, gd)
    cap = max(E, 8)
    host, ref = NH.HostNorm(E, od, gd, capacity=cap), NH.Ref64(E, s.D, cap)
    env = NH.StreamEnv(s)
    tv, tm = VecNormalize(env), EpisodeMonitor(E, torch.device("cpu"), capacity=cap)
    trace = {k: [] for k in ("host", "ref", "torch")}

    def torch_stats():
        return np.concatenate([tv.obs_rms.mean.numpy().astype(np.float64), tv.obs_rms.var.numpy().astype(np.float64),
                               [float(tv.ret_rms.mean), float(tv.ret_rms.var), tv.obs_rms.count, tv.ret_rms.count]])

    trace["host"].append((host.reset(s.parts()), None, host.stats.copy()))
    trace["ref"].append((ref.reset(s.reset_rows), None, ref.stats()))
    trace["torch"].append((tv.reset().numpy(), None, torch_stats()))
    for t in range(s.calls):
        trace["host"].append(host.step(s.parts(t), s.rew[t], s.done[t], s.keep[t], t=float(t)) + (host.stats.copy(),))
        trace["ref"].append(ref.step(s.rows[t], s.rew[t], s.done[t], s.keep[t], t=float(t)) + (ref.stats(),))
        nobs, nrew, done, info, raw = tv.step(None)
        tm.update(raw, done, ~info["resetting"] if "resetting" in info else None)
        trace["torch"].append((nobs.numpy(), nrew.numpy(), torch_stats()))
    _runs[key] = (s, host, ref, tv, tm, trace)
    return _runs[key]


@pytest.mark.parametrize("od,gd", NH.WIDTHS)
@pytest.mark.parametrize("E", SIZES)
def test_host_core_against_float64_numpy(E, od, gd):
    """statistics to 1e-9 absolute (the two differ in float64 summation order only: n u max|x|^2 = 1000 x 1.1e-16 x 16 = 2e-12),
    outputs to one float32 ulp, ring rows equal in order, lengths and n exact"""
    s, host, ref, _, _, trace = run(E, od, gd)
    worst = 0.0
    for k, ((h_obs, h_rew, h_stats), (r_obs, r_rew, r_stats)) in enumerate(zip(trace["host"], trace["ref"])):
        worst = max(worst, float(np.abs(h_stats - r_stats).max()))
        assert np.abs(h_stats - r_stats).max() <= 1e-9, k
        assert bool((np.abs(h_obs.astype(np.float64) - r_obs) <= NH.ulp32(r_obs)).all()), k
        if h_rew is not None:
            assert bool((np.abs(h_rew.astype(np.float64) - r_rew) <= NH.ulp32(r_rew)).all()), k
    print("E %d D %d: largest statistics difference host core - float64 NumPy %.3g" % (E, s.D, worst))
    total = int(sum(int(d.sum()) for d in s.done))
    assert host.n[0] == ref.n == total
    assert host.stats[2 * s.D + 2] == ref.obs[2] and host.stats[2 * s.D + 3] == ref.rr[2]
    assert NH.bits(host.ring) == NH.bits(ref.ring)              # r, l, t of every row, rows in env order, wrapped alike
    assert NH.bits(host.ep_ret) == NH.bits(ref.ep_ret) and NH.bits(host.ep_len) == NH.bits(ref.ep_len)
    assert NH.bits(host.ret) == NH.bits(ref.ret)
    lens = np.asarray(NH.EP_LENS)[np.arange(E) % 7]
    assert np.array_equal(host.ep_len <= lens, np.ones(E, bool))
    if total >= host.cap:
        assert bool((host.ring[:, 1] >= 0).all()) and bool((host.ring[:, 1] <= 5).all())


@pytest.mark.parametrize("od,gd", NH.WIDTHS)
@pytest.mark.parametrize("E", SIZES)
def test_host_core_against_the_torch_classes(E, od, gd):
    """The tolerance comes from the references alone: per quantity, twice the largest deviation of the float32 torch classes
    from the float64 restatement on this stream, plus one float32 ulp at the quantity's largest magnitude.  The monitor's sums
    are the same float32 operations in the same order: exactly equal."""
    s, host, ref, tv, tm, trace = run(E, od, gd)
    D = s.D
    dev = {"nobs": 0.0, "nrew": 0.0, "stats": 0.0}
    mag = {"nobs": 0.0, "nrew": 0.0, "stats": 0.0}
    for (t_obs, t_rew, t_stats), (r_obs, r_rew, r_stats) in zip(trace["torch"], trace["ref"]):
        pairs = [("nobs", t_obs, r_obs), ("stats", t_stats[:2 * D + 2], r_stats[:2 * D + 2])] + ([("nrew", t_rew, r_rew)] if t_rew is not None else [])
        for k, a, b in pairs:
            dev[k] = max(dev[k], float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()))
            mag[k] = max(mag[k], float(np.abs(b).max()))
    tol = {k: 2.0 * dev[k] + float(NH.ulp32(mag[k])) for k in dev}
    print("E %d D %d: torch float32 classes - float64 restatement, largest deviation %s; tolerance %s" % (E, D, dev, tol))
    for k, ((h_obs, h_rew, h_stats), (t_obs, t_rew, t_stats)) in enumerate(zip(trace["host"], trace["torch"])):
        assert np.abs(h_obs.astype(np.float64) - t_obs).max() <= tol["nobs"], k
        assert np.abs(h_stats[:2 * D + 2] - t_stats[:2 * D + 2]).max() <= tol["stats"], k
        assert h_stats[2 * D + 2] == t_stats[2 * D + 2] and h_stats[2 * D + 3] == t_stats[2 * D + 3], k   # counts: float64 in both
        if h_rew is not None:
            assert np.abs(h_rew.astype(np.float64) - t_rew).max() <= tol["nrew"], k
    assert host.n[0] == tm.n
    assert NH.bits(host.ep_ret) == NH.bits(tm.ep_ret.numpy()) and NH.bits(host.ep_len) == NH.bits(tm.ep_len.numpy())
    assert NH.bits(host.ring[:, :2]) == NH.bits(tm.ring[:host.cap, :2].numpy())


def test_statistics_do_not_move_without_kept_rows_or_with_training_off():
    s = NH.Stream(129, 24, 3, calls=6)
    host = NH.HostNorm(129, 24, 3)
    host.reset(s.parts())
    host.step(s.parts(0), s.rew[0], s.done[0])
    before = host.stats.copy()
    assert not np.array_equal(before, NH.new_stats(s.D))
    none = np.zeros(129, np.uint8)
    len0 = host.ep_len.copy()
    nobs, nrew = host.step(s.parts(1), s.rew[1], s.done[1], none)               # no kept row
    assert NH.bits(host.stats) == NH.bits(before)
    assert bool(np.isfinite(nobs).all()) and bool(np.isfinite(nrew).all())
    assert np.array_equal(host.ep_len, np.where(s.done[1] != 0, 0, len0))        # the dropped call adds no length
    host.training = False
    n0 = int(host.n[0])
    nobs, nrew = host.step(s.parts(2), s.rew[2], s.done[2])
    assert NH.bits(host.stats) == NH.bits(before)
    D = s.D
    expect = np.clip((s.rows[2].astype(np.float64) - before[:D]) / np.sqrt(before[D:2 * D] + 1e-8), -10, 10).astype(np.float32)
    assert NH.bits(nobs) == NH.bits(expect)                                     # the loaded values normalise
    expect = np.clip(s.rew[2].astype(np.float64) / np.sqrt(before[2 * D + 1] + 1e-8), -10, 10).astype(np.float32)
    assert NH.bits(nrew) == NH.bits(expect)
    assert int(host.n[0]) == n0 + int(s.done[2].sum())                          # the monitor still records
    assert NH.bits(host.reset(s.parts(3))) == NH.bits(np.clip((s.rows[3].astype(np.float64) - before[:D]) / np.sqrt(before[D:2 * D] + 1e-8), -10, 10).astype(np.float32))
    assert NH.bits(host.stats) == NH.bits(before) and not host.ret.any()


class CpuEnv:
    device, num_envs, obs_dim, goal_dim, act_dim = torch.device("cpu"), 5, 8, 3, 4


def test_state_moves_between_the_two_classes_in_both_directions(tmp_path):
    from gym_xarm_amd.normalize import DeviceVecNormalize
    g = torch.Generator().manual_seed(0)
    tv = VecNormalize(CpuEnv(), clip_obs=7.0, clip_reward=3.0, gamma=0.9)
    tv.obs_rms.mean, tv.obs_rms.var, tv.obs_rms.count = torch.randn(14, generator=g), torch.rand(14, generator=g) + 0.5, 1234.0001
    tv.ret_rms.mean, tv.ret_rms.var, tv.ret_rms.count = torch.tensor(0.25), torch.tensor(2.5), 77.0001
    dv = DeviceVecNormalize(CpuEnv())
    dv.load_state_dict(tv.state_dict())                                       # torch -> device: float32 values, exactly
    assert torch.equal(dv.obs_mean, tv.obs_rms.mean.double()) and torch.equal(dv.obs_var, tv.obs_rms.var.double())
    assert dv.stats[28:].tolist() == [0.25, 2.5, 1234.0001, 77.0001]
    assert (dv.clip_obs, dv.clip_reward) == (7.0, 3.0) and dv.gamma == float(torch.tensor(0.9))
    sd_t, sd_d = tv.state_dict(), dv.state_dict()
    assert set(sd_t) <= set(sd_d) and set(sd_d) - set(sd_t) == {"obs_mean_f64", "obs_var_f64", "ret_mean_f64", "ret_var_f64"}
    for k in sd_t:
        assert sd_d[k].dtype == sd_t[k].dtype and sd_d[k].shape == sd_t[k].shape and torch.equal(sd_d[k], sd_t[k]), k
    # device -> file -> both classes; float64 statistics that float32 cannot hold survive the device class's own round trip
    dv.stats[:14] += 1e-11
    dv.save(str(tmp_path / "d.safetensors"))
    back = DeviceVecNormalize.load(str(tmp_path / "d.safetensors"), CpuEnv())
    assert torch.equal(back.stats, dv.stats) and back.gamma == dv.gamma and back.clip_obs == 7.0
    t2 = VecNormalize.load(str(tmp_path / "d.safetensors"), CpuEnv())
    assert torch.equal(t2.obs_rms.mean, dv.obs_mean.float()) and torch.equal(t2.obs_rms.var, dv.obs_var.float())
    assert t2.obs_rms.count == 1234.0001 and t2.ret_rms.count == 77.0001 and float(t2.ret_rms.var) == 2.5 and t2.clip_obs == 7.0
    # torch -> file -> device
    tv.save(str(tmp_path / "t.safetensors"))
    d3 = DeviceVecNormalize.load(str(tmp_path / "t.safetensors"), CpuEnv())
    assert torch.equal(d3.obs_mean, tv.obs_rms.mean.double()) and d3.stats[28:].tolist() == [0.25, 2.5, 1234.0001, 77.0001]
    with pytest.raises(ValueError, match="width"):
        DeviceVecNormalize(type("E", (CpuEnv,), {"obs_dim": 9})()).load_state_dict(tv.state_dict())
    # save_model / load_model take the device class as they take the torch class
    from gym_xarm_amd.train import ActorCritic, load_model, save_model
    model = ActorCritic(14, 4)
    save_model(str(tmp_path / "m.safetensors"), model, dv)
    d4, t4 = DeviceVecNormalize(CpuEnv()), VecNormalize(CpuEnv())
    load_model(str(tmp_path / "m.safetensors"), ActorCritic(14, 4), d4)
    load_model(str(tmp_path / "m.safetensors"), ActorCritic(14, 4), t4)
    assert torch.equal(d4.stats, dv.stats) and torch.equal(t4.obs_rms.mean, dv.obs_mean.float())


def test_device_class_has_no_host_path_and_refuses_a_small_ring():
    from gym_xarm_amd.normalize import DeviceVecNormalize
    with pytest.raises(ValueError, match="no host path"):
        DeviceVecNormalize(CpuEnv()).reset()
    with pytest.raises(ValueError, match="monitor_capacity"):
        DeviceVecNormalize(CpuEnv(), monitor_capacity=4)
    with pytest.raises(RuntimeError):
        DeviceVecNormalize(CpuEnv()).monitor.update(None, None)


def test_abi_argument_errors():
    from gym_xarm_amd import _native
    L = _native.load()
    lay = lambda *a: C.byref(_native.XarmNormLayout(*a))
    par = lambda clip_obs=10.0, clip_reward=10.0, eps=1e-8, gamma=0.99, update=1: C.byref(
        _native.XarmNormParams(clip_obs, clip_reward, eps, gamma, 0.0, update))
    err = lambda: L.xarm_last_error(None).decode()
    nbytes = C.c_int64(0)
    good = lay(1000, 24, 3, 1000)
    assert L.xarm_norm_work_bytes(good, C.byref(nbytes)) == 0
    assert nbytes.value == 8 * (8 * (2 * 31 + 1) + 2 * 8 + 1)                   # 8 chunks of 128
    assert L.xarm_norm_work_bytes(good, None) == -1 and "NULL" in err()
    assert L.xarm_norm_work_bytes(None, C.byref(nbytes)) == -1 and "NULL" in err()
    obs = lambda l, p, ptrs=(None,) * 6, zero_ret=0: L.xarm_norm_obs(l, p, *ptrs, zero_ret, None, None)
    step = lambda l, p: L.xarm_norm_step(l, p, *([None] * 16))
    for bad, word in (((-1, 24, 3, 1000), "num_envs"), ((1000, 0, 3, 1000), "obs_dim"), ((1000, 24, -1, 1000), "goal_dim"),
                      ((1000, 24, 3, 999), "monitor_capacity"), ((0, 24, 3, 0), "monitor_capacity"), ((8, 95, 1, 8), "XARM_NORM_MAX_DIM"),
                      ((8, 97, 0, 8), "XARM_NORM_MAX_DIM")):
        assert L.xarm_norm_work_bytes(lay(*bad), C.byref(nbytes)) == -1 and word in err(), bad
        assert obs(lay(*bad), par()) == -1 and word in err(), bad
        assert step(lay(*bad), par()) == -1 and word in err(), bad
    assert L.xarm_norm_work_bytes(lay(8, 96, 0, 8), C.byref(nbytes)) == 0
    for kw, word in ((dict(eps=0.0), "eps"), (dict(eps=-1e-8), "eps"), (dict(eps=float("inf")), "eps"), (dict(eps=float("nan")), "eps"),
                     (dict(clip_obs=0.0), "clip_obs"), (dict(clip_obs=-1.0), "clip_obs"), (dict(clip_obs=float("nan")), "clip_obs"),
                     (dict(clip_reward=0.0), "clip_reward"), (dict(gamma=-0.01), "gamma"), (dict(gamma=1.01), "gamma"),
                     (dict(gamma=float("nan")), "gamma")):
        assert obs(good, par(**kw)) == -1 and word in err(), kw
        assert step(good, par(**kw)) == -1 and word in err(), kw
    assert obs(good, None) == -1 and "params" in err()
    assert step(good, None) == -1 and "params" in err()
    assert obs(good, par()) == -1 and "xarm_norm_obs: NULL pointer" in err()
    assert step(good, par()) == -1 and "xarm_norm_step: NULL pointer" in err()
    # each pointer a path reads or writes, one at a time (any non-null value: the check comes before any launch)
    x = C.c_void_p(64)
    obs_args = lambda **nulls: L.xarm_norm_obs(nulls.pop("layout", good), par(), *[None if k in nulls else x for k in ("stats", "ret", "work", "obs", "ag", "dg")],
                                               nulls.pop("zero_ret", 1), None if "nobs" in nulls else x, None)
    for k in ("stats", "ret", "work", "obs", "ag", "dg", "nobs"):
        assert obs_args(**{k: 1}) == -1 and "NULL pointer" in err(), k
    names = ("stats", "ret", "ep_ret", "ep_len", "ring", "n", "work", "obs", "ag", "dg", "rew", "done", "keep", "nobs", "nrew")
    for k in names:
        if k != "keep":                                                     # keep may be NULL
            rc = L.xarm_norm_step(good, par(), *[None if n == k else x for n in names], None)
            assert rc == -1 and "NULL pointer" in err(), k
    # no env: nothing to launch, nothing read
    empty = lay(0, 24, 3, 1)
    assert obs(empty, par()) == 0 and step(empty, par()) == 0
    assert L.xarm_norm_work_bytes(empty, C.byref(nbytes)) == 0 and nbytes.value == 8
    assert _native.NORM_MAX_DIM == 96 and C.sizeof(_native.XarmNormLayout) == 16 and C.sizeof(_native.XarmNormParams) == 40


def _have_sanitizers():
    """libasan / libubsan are installed and a sanitized program starts in this environment"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "san_probe")
        return subprocess.run(["g++", "-x", "c++", "-", "-fsanitize=address,undefined", "-o", exe], input=b"int main(){return 0;}",
                              capture_output=True).returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason="libasan/libubsan not available")
def test_host_core_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the scripted stream through the host core as a stand-alone program (its own main, never loaded into python)"""
    exe = str(tmp_path / "norm_main_san")
    src = os.path.join(NH.DIR, "norm_main.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "norm_main ok" in r.stdout and "ERROR" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
