"""ctypes view of tests/hostbuild_norm (g++ -ffp-contract=off build of csrc/xarm_norm_core.h) - CPU-side tests only - with the
scripted stream, the float64 NumPy restatement of train.py's VecNormalize / EpisodeMonitor and the torch-side stand-in env that
the host and GPU normaliser tests share."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "hostbuild_norm")
WIDTHS = ((8, 3), (24, 3), (29, 0), (68, 12))     # Reach, PickAndPlace, a flat row, Rearrange
EP_LENS = (3, 4, 5, 5, 2, 4, 1)
GXX_FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]
_lib = None


def sources():
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    return [os.path.join(DIR, "norm_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h"), os.path.join(csrc, "xarm_norm_core.h")]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "libnorm_host.so")
    srcs = sources()
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + GXX_FLAGS + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.nh_work_bytes.argtypes = [vp]
    L.nh_work_bytes.restype = C.c_int64
    L.nh_obs.argtypes = [vp] * 8 + [C.c_int32, vp]
    L.nh_step.argtypes = [vp] * 17
    _lib = L
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def new_stats(D):
    s = np.zeros(2 * D + 4, np.float64)
    s[D:2 * D] = 1.0
    s[2 * D + 1] = 1.0
    s[2 * D + 2:] = 1e-4
    return s


class HostNorm:
    """the normaliser + monitor of csrc/xarm_norm_core.h on NumPy arrays (same state arrays as DeviceVecNormalize)"""

    def __init__(self, E, obs_dim, goal_dim, capacity=None, clip_obs=10.0, clip_reward=10.0, gamma=0.99, eps=1e-8):
        from gym_xarm_amd import _native
        self.E, self.obs_dim, self.goal_dim, self.D = E, obs_dim, goal_dim, obs_dim + 2 * goal_dim
        self.cap = max(E, 1) if capacity is None else capacity
        self.layout = _native.XarmNormLayout(E, obs_dim, goal_dim, self.cap)
        self.clip_obs, self.clip_reward, self.gamma, self.eps, self.training = clip_obs, clip_reward, gamma, eps, True
        self._native = _native
        nbytes = lib().nh_work_bytes(C.byref(self.layout))
        assert nbytes > 0 and nbytes % 8 == 0
        self.work = np.zeros(nbytes // 8, np.int64)
        self.stats = new_stats(self.D)
        self.ret, self.ep_ret, self.ep_len = (np.zeros(E, np.float32) for _ in range(3))
        self.ring = np.zeros((self.cap, 3), np.float32)
        self.n = np.zeros(1, np.int64)

    def params(self, t=0.0):
        return self._native.XarmNormParams(self.clip_obs, self.clip_reward, self.eps, self.gamma, t, int(self.training))

    def poison(self, nobs=None, nrew=None):
        """NaN / 0xFF in the workspace and the outputs: every element must be written, nothing stale read"""
        self.work.view(np.uint8)[:] = 0xFF
        for x in (nobs, nrew):
            if x is not None:
                x[...] = np.nan

    def reset(self, parts, zero_ret=True):
        nobs = np.full((self.E, self.D), np.nan, np.float32)
        self.poison()
        rc = lib().nh_obs(C.byref(self.layout), C.byref(self.params()), _p(self.stats), _p(self.ret), _p(self.work),
                          *[_p(x) for x in parts], int(zero_ret), _p(nobs))
        assert rc == 0
        return nobs

    def step(self, parts, rew, done, keep=None, t=0.0):
        nobs, nrew = np.full((self.E, self.D), np.nan, np.float32), np.full(self.E, np.nan, np.float32)
        self.poison()
        rc = lib().nh_step(C.byref(self.layout), C.byref(self.params(t)), _p(self.stats), _p(self.ret), _p(self.ep_ret), _p(self.ep_len),
                           _p(self.ring), _p(self.n), _p(self.work), *[_p(x) for x in parts], _p(rew), _p(done), _p(keep), _p(nobs), _p(nrew))
        assert rc == 0
        return nobs, nrew


def split(rows, obs_dim, goal_dim):
    """a [E, D] row set as the call's three inputs (None for the goal parts of a flat row)"""
    c = np.ascontiguousarray
    if goal_dim == 0:
        return [c(rows), None, None]
    return [c(rows[:, :obs_dim]), c(rows[:, obs_dim:obs_dim + goal_dim]), c(rows[:, obs_dim + goal_dim:])]


class Stream:
    """the scripted stream: a reset row set, then `calls` steps with |obs| <= 4, |rew| <= 4, env e finishing an episode every
    EP_LENS[e % 7] calls, and on every third call a keep mask that drops every fifth row.  done_mode / keep_mode replace the
    script's masks (the GPU cases): done 'none' | 'all' | 'edge' (the last env of one chunk and the first of the next, clipped to
    the batch), keep 'none' | 'mixed' | 'dropped'."""

    def __init__(self, E, obs_dim, goal_dim, calls=30, seed=0, done_mode=None, keep_mode=None):
        rng = np.random.RandomState(1000 * seed + E + 7 * obs_dim)
        D = obs_dim + 2 * goal_dim
        self.E, self.obs_dim, self.goal_dim, self.D, self.calls = E, obs_dim, goal_dim, D, calls
        self.reset_rows = rng.uniform(-4, 4, (E, D)).astype(np.float32)
        self.rows = rng.uniform(-4, 4, (calls, E, D)).astype(np.float32)
        self.rew = rng.uniform(-4, 4, (calls, E)).astype(np.float32)
        e = np.arange(E)
        lens = np.asarray(EP_LENS)[e % 7]
        self.done, self.keep = [], []
        for t in range(1, calls + 1):
            d = (t % lens == 0)
            if done_mode == "none":
                d = np.zeros(E, bool)
            elif done_mode == "all":
                d = np.ones(E, bool)
            elif done_mode == "edge":
                d = np.zeros(E, bool)
                d[[min(127, E - 1), min(128, E - 1)]] = True
            k = (e % 5 != 4) if t % 3 == 2 else None
            if keep_mode == "none":
                k = None
            elif keep_mode == "mixed":
                k = (e + t) % 3 != 0
            elif keep_mode == "dropped":
                k = np.zeros(E, bool)
            self.done.append(d.astype(np.uint8))
            self.keep.append(None if k is None else k.astype(np.uint8))

    def parts(self, t=None):
        return split(self.reset_rows if t is None else self.rows[t], self.obs_dim, self.goal_dim)


class Ref64:
    """train.py's RunningMeanStd / VecNormalize / EpisodeMonitor restated in NumPy: float64 statistics and normalisation, and
    the float32 operations the specification names (ret = ret * gamma + rew, ep_ret += rew * c, ep_len += c) in float32"""

    def __init__(self, E, D, cap, clip_obs=10.0, clip_reward=10.0, gamma=0.99, eps=1e-8):
        self.E, self.D, self.cap, self.clip_obs, self.clip_reward, self.gamma, self.eps = E, D, cap, clip_obs, clip_reward, gamma, eps
        self.obs = [np.zeros(D), np.ones(D), 1e-4]
        self.rr = [np.zeros(()), np.ones(()), 1e-4]
        self.ret, self.ep_ret, self.ep_len = (np.zeros(E, np.float32) for _ in range(3))
        self.ring, self.n, self.training = np.zeros((cap, 3), np.float32), 0, True

    @staticmethod
    def update(rms, x):
        x = x.astype(np.float64)
        b_mean, b_var, b_n = x.mean(0), x.var(0), x.shape[0]
        mean, var, count = rms
        delta, tot = b_mean - mean, count + b_n
        rms[0] = mean + delta * b_n / tot
        rms[1] = (var * count + b_var * b_n + delta ** 2 * count * b_n / tot) / tot
        rms[2] = tot

    def stats(self):
        return np.concatenate([self.obs[0], self.obs[1], [self.rr[0], self.rr[1], self.obs[2], self.rr[2]]])

    def norm(self, x, keep=None):
        if self.training:
            rows = x if keep is None else x[keep]
            if rows.shape[0] > 0:
                self.update(self.obs, rows)
        return np.clip((x.astype(np.float64) - self.obs[0]) / np.sqrt(self.obs[1] + self.eps), -self.clip_obs, self.clip_obs).astype(np.float32)

    def reset(self, x):
        self.ret[:] = 0
        return self.norm(x)

    def step(self, x, rew, done, keep=None, t=0.0):
        keep = None if keep is None else keep != 0
        self.ret = self.ret * np.float32(self.gamma) + rew
        assert self.ret.dtype == np.float32
        if self.training:
            r = self.ret if keep is None else self.ret[keep]
            if r.shape[0] > 0:
                self.update(self.rr, r)
        nrew = np.clip(rew.astype(np.float64) / np.sqrt(self.rr[1] + self.eps), -self.clip_reward, self.clip_reward).astype(np.float32)
        fin = done != 0
        self.ret = np.where(fin, np.float32(0), self.ret)
        nobs = self.norm(x, keep)
        c = np.ones(self.E, np.float32) if keep is None else keep.astype(np.float32)
        self.ep_ret = self.ep_ret + rew * c
        self.ep_len = self.ep_len + c
        for e in np.nonzero(fin)[0]:
            self.ring[self.n % self.cap] = (self.ep_ret[e], self.ep_len[e], np.float32(t))
            self.n += 1
        self.ep_ret = np.where(fin, np.float32(0), self.ep_ret)
        self.ep_len = np.where(fin, np.float32(0), self.ep_len)
        return nobs, nrew


class StreamEnv:
    """torch-side stand-in that plays a Stream to train.py's VecNormalize: dict observations (a flat tensor for goal_dim 0),
    info['resetting'] = the dropped rows on the calls that carry a keep mask"""

    def __init__(self, stream, device="cpu"):
        self.s, self.device, self.t = stream, torch.device(device), 0
        self.num_envs, self.obs_dim, self.goal_dim, self.act_dim = stream.E, stream.obs_dim, stream.goal_dim, 1
        self.flat_observation = stream.goal_dim == 0

    def _obs(self, parts):
        t = [None if p is None else torch.from_numpy(p).to(self.device) for p in parts]
        return t[0] if self.flat_observation else {"observation": t[0], "achieved_goal": t[1], "desired_goal": t[2]}

    def reset(self):
        self.t = 0
        return self._obs(self.s.parts())

    def step(self, actions):
        t = self.t
        self.t += 1
        info = {}
        if self.s.keep[t] is not None:
            info["resetting"] = torch.from_numpy(self.s.keep[t] == 0).to(self.device)
        return (self._obs(self.s.parts(t)), torch.from_numpy(self.s.rew[t]).to(self.device),
                torch.from_numpy(self.s.done[t]).to(self.device), info)

    def close(self):
        pass


def ulp32(x):
    """one float32 unit in the last place at the magnitude of x"""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def bits(x):
    return np.ascontiguousarray(x).tobytes()
