"""ctypes view of tests/hostbuild_replay (g++ build of csrc/xarm_replay_core.h) - CPU-side replay tests only - and the scripted
streams the host and GPU uniform-replay tests share."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

from her_host import ScriptedEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "hostbuild_replay")
GXX_FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]
OUT = (("obs", "D", np.float32), ("next_obs", "D", np.float32), ("action", "act", np.float32), ("reward", None, np.float32),
       ("done", None, np.float32), ("use", None, np.float32), ("env", None, np.int64), ("time", None, np.int64))
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "libreplay_host.so")
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    srcs = [os.path.join(DIR, "replay_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + [
        os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + GXX_FLAGS + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.rh_record_floats.argtypes = [vp]
    L.rh_add.argtypes = [vp] * 12
    L.rh_sample.argtypes = [vp, vp, vp, C.c_uint64, C.c_int32, C.c_int32, vp, C.c_double, C.c_double] + [vp] * 8
    _lib = L
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class HostReplay:
    """the uniform replay buffer of csrc/xarm_replay_core.h on NumPy arrays"""

    def __init__(self, E, horizon, obs_dim, goal_dim, act_dim, seed=0, handle_timeout=True):
        from gym_xarm_amd import _native
        self.E, self.T, self.D = E, horizon, obs_dim + 2 * goal_dim
        self.dims = dict(D=self.D, act=act_dim)
        self.obs_dim, self.goal_dim, self.act_dim = obs_dim, goal_dim, act_dim
        self.layout = _native.XarmReplayLayout(E, horizon, obs_dim, goal_dim, act_dim)
        self.R = lib().rh_record_floats(C.byref(self.layout))
        assert self.R == 2 * self.D + act_dim + 3
        self.ring = np.zeros((horizon, E, self.R), np.float32)
        self.clock = np.zeros(2, np.int64)
        self.seed, self.handle_timeout = seed, handle_timeout

    def add(self, obs, next_obs, action, reward, done, timeout=None):
        f = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        u8 = lambda x: np.ascontiguousarray(np.asarray(x) != 0, dtype=np.uint8)
        if self.goal_dim == 0:
            parts = [f(obs), None, None, f(next_obs), None]
        else:
            parts = [f(obs["observation"]), f(obs["achieved_goal"]), f(obs["desired_goal"]), f(next_obs["observation"]),
                     f(next_obs["achieved_goal"])]
        rest = [f(action), f(reward), u8(done), None if timeout is None else u8(timeout)]
        rc = lib().rh_add(C.byref(self.layout), _p(self.ring), _p(self.clock), *[_p(x) for x in parts + rest])
        assert rc == 0

    def sample(self, B, stats=None, clip_obs=10.0, eps=1e-8, handle_timeout=None):
        out = {k: np.full((B, self.dims[d]) if d else (B,), 77, dtype=t) for k, d, t in OUT}   # 77: every element must be written
        ht = self.handle_timeout if handle_timeout is None else handle_timeout
        st = None if stats is None else np.ascontiguousarray(stats, dtype=np.float64)
        rc = lib().rh_sample(C.byref(self.layout), _p(self.ring), _p(self.clock), self.seed, B, int(ht), _p(st), clip_obs, eps,
                             *[_p(out[k]) for k, _, _ in OUT])
        assert rc == 0
        return out


class FlatScripted:
    """ScriptedEnv behind the flat-observation view: the observation tensor alone, as sb3_adapter.FlatObsVecEnv hands it out.
    Env e's episodes end by truncation when e is even and by termination when e is odd (info["TimeLimit.truncated"])."""

    flat_observation = True

    def __init__(self, ep_len, obs_dim=5, act_dim=3, device="cpu"):
        self.env = ScriptedEnv(ep_len, obs_dim=obs_dim, goal_dim=3, act_dim=act_dim, device=device)
        self.num_envs, self.device = self.env.num_envs, self.env.device
        self.obs_dim, self.goal_dim, self.act_dim, self.action_dim = obs_dim, 0, act_dim, act_dim
        self.max_episode_steps = self.env.max_episode_steps

    def policy(self, obs):
        return self.env.policy(obs)

    def reset(self):
        return self.env.reset()["observation"]

    def step(self, act):
        obs, rew, done, info = self.env.step(act)
        info["TimeLimit.truncated"] = (done != 0) & (torch.arange(self.num_envs) % 2 == 0)
        info["is_success"] = ((done != 0) & ~info["TimeLimit.truncated"]).to(torch.float32)
        return obs["observation"], rew, done, info

    def close(self):
        pass


class GoalScripted(ScriptedEnv):
    """ScriptedEnv with the truncation flag and what the training driver reads"""

    def step(self, act):
        obs, rew, done, info = super().step(act)
        info["TimeLimit.truncated"] = (done != 0) & (torch.arange(self.num_envs) % 2 == 0)
        info["is_success"] = ((done != 0) & ~info["TimeLimit.truncated"]).to(torch.float32)
        return obs, rew, done, info

    def close(self):
        pass


def collect(env, buffers, steps, obs=None):
    """roll `steps` steps of a FlatScripted / GoalScripted env with its scripted policy into every buffer of `buffers`, the way the
    training driver stores them: the previous observation cloned, the terminal observation for finished envs, the truncation flag"""
    flat = bool(getattr(env, "flat_observation", False))
    if obs is None:
        obs = env.reset()
    for _ in range(steps):
        prev = obs.clone() if flat else {k: v.clone() for k, v in obs.items()}
        act = env.policy(prev)
        obs, rew, done, info = env.step(act)
        d = (done != 0)[:, None]
        term = info["terminal_observation"]
        if flat:
            nxt = torch.where(d, term, obs)
        else:
            nxt = {"observation": torch.where(d, term, obs["observation"]),
                   "achieved_goal": torch.where(d, env.achieved_goal_of(term), obs["achieved_goal"])}
        for b in buffers:
            b.add(prev, nxt, act, rew, done, info["TimeLimit.truncated"])
    return obs


def ep_lens(E):
    return [(3, 4, 5, 5, 2, 4, 1)[e % 7] for e in range(E)]
