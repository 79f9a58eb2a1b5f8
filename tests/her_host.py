"""ctypes view of tests/hostbuild_her (g++ build of csrc/xarm_her_core.h) - CPU-side replay tests only - and the scripted
transition stream the host and GPU replay tests share."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "hostbuild_her")
STRATEGY = {"future": 0, "final": 1, "episode": 2}
OUT = (("observation", "obs", np.float32), ("next_observation", "obs", np.float32), ("achieved_goal", "goal", np.float32),
       ("next_achieved_goal", "goal", np.float32), ("desired_goal", "goal", np.float32), ("action", "act", np.float32),
       ("reward", None, np.float32), ("done", None, np.uint8), ("env", None, np.int64), ("time", None, np.int64),
       ("goal_time", None, np.int64), ("ok", None, np.uint8))
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "libher_host.so")
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    srcs = [os.path.join(DIR, "her_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + [
        os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.hh_record_floats.argtypes = [vp]
    L.hh_add.argtypes = [vp] * 14
    L.hh_sample.argtypes = [vp] * 5 + [C.c_uint64, C.c_int32, C.c_int32, C.c_int32] + [vp] * 13
    _lib = L
    return L


def _p(a):
    return C.c_void_p(a.ctypes.data)


class HostHer:
    """the replay buffer of csrc/xarm_her_core.h on NumPy arrays"""

    def __init__(self, E, horizon, obs_dim, goal_dim, act_dim, seed=0, n_sampled_goal=4, strategy="future"):
        from gym_xarm_amd import _native
        self.E, self.T, self.dims = E, horizon, dict(obs=obs_dim, goal=goal_dim, act=act_dim)
        self.layout = _native.XarmHerLayout(E, horizon, obs_dim, goal_dim, act_dim)
        self.R = lib().hh_record_floats(C.byref(self.layout))
        assert self.R == 2 * obs_dim + 3 * goal_dim + act_dim + 2
        self.ring = np.zeros((horizon, E, self.R), np.float32)
        self.ep_end = np.full((horizon, E), -1, np.int64)
        self.ep_first = np.full((horizon, E), -1, np.int64)
        self.ep_start = np.zeros(E, np.int64)
        self.clock = np.zeros(2, np.int64)
        self.fail_count = np.zeros(1, np.int64)
        self.seed, self.strategy, self.her_ratio = seed, strategy, 1.0 - 1.0 / (n_sampled_goal + 1)

    def add(self, obs, next_obs, action, reward, done):
        f = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float32))
        a = [f(obs["observation"]), f(next_obs["observation"]), f(obs["achieved_goal"]), f(next_obs["achieved_goal"]),
             f(obs["desired_goal"]), f(action), f(reward), np.ascontiguousarray(np.asarray(done) != 0, dtype=np.uint8)]
        rc = lib().hh_add(C.byref(self.layout), _p(self.ring), _p(self.ep_end), _p(self.ep_first), _p(self.ep_start), _p(self.clock),
                          *[_p(x) for x in a])
        assert rc == 0

    def sample(self, B, strategy=None):
        out = {k: np.full((B, self.dims[d]) if d else (B,), 77, dtype=t) for k, d, t in OUT}   # 77: every element must be written
        n_her = int(round(self.her_ratio * B))
        rc = lib().hh_sample(C.byref(self.layout), _p(self.ring), _p(self.ep_end), _p(self.ep_first), _p(self.clock), self.seed,
                             STRATEGY[strategy or self.strategy], B, n_her, *[_p(out[k]) for k, _, _ in OUT], _p(self.fail_count))
        assert rc == 0
        out["n_her"] = n_her
        return out


class ScriptedEnv:
    """host stand-in with the attributes the buffers read.  Env e ends an episode every ep_len[e] steps; the achieved goal is
    (env, absolute time, steps into the episode) so that every sampled field can be traced to its source transition, and
    observation, desired goal, action and reward are distinct functions of (env, time) too."""

    def __init__(self, ep_len, obs_dim=4, goal_dim=3, act_dim=2, device="cpu"):
        self.ep_len = torch.as_tensor(ep_len, dtype=torch.int64)
        self.num_envs, self.device = len(ep_len), torch.device(device)   # the tensors stay on the host: `device` is what a buffer is told
        self.obs_dim, self.goal_dim, self.action_dim, self.act_dim = obs_dim, goal_dim, act_dim, act_dim
        self.max_episode_steps = int(self.ep_len.max())
        self.t = 0
        self.steps = torch.zeros(self.num_envs, dtype=torch.int64)

    def compute_reward(self, ag, g, info):
        return (torch.linalg.norm(ag - g, dim=-1) < 0.05).to(torch.float32)

    def achieved_goal_of(self, obs):
        return obs[..., 0:self.goal_dim]

    def _obs(self):
        e = torch.arange(self.num_envs, dtype=torch.float32)
        ag = torch.zeros(self.num_envs, self.goal_dim)
        ag[:, 0], ag[:, 1], ag[:, 2] = e, float(self.t), self.steps.to(torch.float32)
        ag[:, 3:] = torch.arange(3, self.goal_dim, dtype=torch.float32) * 0.5 + e[:, None]
        rest = torch.arange(self.obs_dim - self.goal_dim, dtype=torch.float32)[None, :] * 100.0 + e[:, None] + 1000.0 * self.t
        return {"observation": torch.cat([ag, rest], 1), "achieved_goal": ag,
                "desired_goal": -1.0 - e[:, None] - torch.arange(self.goal_dim, dtype=torch.float32)[None, :] / 16}

    def policy(self, obs):
        e = torch.arange(self.num_envs, dtype=torch.float32)
        return (e[:, None] * 8 + torch.arange(self.act_dim, dtype=torch.float32)[None, :]) + 0.25 * self.t

    def reset(self):
        return self._obs()

    def step(self, act):
        self.t += 1
        self.steps += 1
        done = self.steps >= self.ep_len
        term = self._obs()["observation"]
        self.steps = torch.where(done, torch.zeros_like(self.steps), self.steps)
        rew = torch.arange(self.num_envs, dtype=torch.float32) / 4 - float(self.t)
        return self._obs(), rew, done.to(torch.uint8), {"terminal_observation": term}


class Tee:
    """feeds every add to several buffers; after_add(t) runs after each one"""

    def __init__(self, buffers, after_add=None):
        self.buffers, self.after_add, self.n = buffers, after_add, 0

    def add(self, *a):
        for b in self.buffers:
            b.add(*a)
        self.n += 1
        if self.after_add:
            self.after_add(self.n)


def ep_lens(E):
    """the episode lengths of tests/test_her.py's FakeEnv, one env of length 1, repeated to E envs"""
    return [(3, 4, 5, 5, 2, 4, 1)[e % 7] for e in range(E)]
