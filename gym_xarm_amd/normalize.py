"""Device-resident VecNormalize + episode monitor: train.py's `VecNormalize` and `EpisodeMonitor` as one fused HIP call per
env step (csrc/xarm_k_norm.hip).

The torch classes of train.py restate SB3's wrapper in ~40 small launches per step, with part of their state on the host
(`count` is a Python float, the statistics tensors are rebound every call), so they can be neither cheap at small batches nor
captured in a graph.  `DeviceVecNormalize` keeps everything - float64 statistics, discounted return, per-env episode return /
length, the ring of finished episodes and its counter - in device tensors that are updated in place by three launches:
per-chunk moments, an in-order merge, and the apply pass that also concatenates observation | achieved_goal | desired_goal.
The torch classes stay as they are and are the checker (tests/test_norm_host.py, tests/test_norm_gpu.py).
"""
import ctypes as C
import json
import os
import time

import torch

from . import _native
from .train import EpisodeMonitor


class DeviceEpisodeMonitor(EpisodeMonitor):
    """EpisodeMonitor's surface (n, ep_ret, last, mean_reward, flush, t_start, the Monitor CSV) on the tensors that
    DeviceVecNormalize's step call updates: there is no `update` to call, and the ring has no dump slot (an env that does not
    finish writes no row)."""

    def __init__(self, num_envs, device, log_dir=None, env_id="", capacity=1 << 20):
        self.dev, self.log_dir, self.env_id, self.cap = device, log_dir, env_id, int(capacity)
        self.ep_ret = torch.zeros(num_envs, device=device)
        self.ep_len = torch.zeros(num_envs, device=device)
        self.ring = torch.zeros(self.cap, 3, device=device)
        self.n_dev = torch.zeros(1, dtype=torch.long, device=device)
        self.flushed = 0
        self.t_start = time.time()
        self._file = None
        if log_dir is not None:
            os.makedirs(log_dir, exist_ok=True)
            self._file = os.path.join(log_dir, "0.monitor.csv")
            with open(self._file, "w") as f:
                f.write("#%s\n" % json.dumps({"t_start": self.t_start, "env_id": env_id}))
                f.write("r,l,t\n")

    def update(self, raw_reward, done, count=None):
        raise RuntimeError("DeviceEpisodeMonitor is updated by DeviceVecNormalize.step / step_into, in the same kernels")


class DeviceVecNormalize:
    """VecNormalize(norm_obs, norm_reward, clip_obs) + Monitor with the state on the device and the step in HIP kernels.

    Same surface as train.py's VecNormalize (`reset`, `step` -> (nobs, nrew, done, info, raw), `training`, `dim`, `flat`,
    `state_dict`, `load_state_dict`, `save`, `load`) and, as `.monitor`, EpisodeMonitor's.  The statistics are float64
    (`stats`: obs_mean[D] | obs_var[D] | ret_mean | ret_var | obs_count | ret_count); `state_dict` hands out VecNormalize's keys
    and dtypes plus exact `*_f64` copies that `load_state_dict` prefers and the torch class ignores, so files move between the
    two classes in both directions.

    `step_into(out, obs, rew, done, keep)` is the call itself on caller-owned tensors: no allocation, no host read, three
    launches on the current stream, so it can be captured in a torch.cuda.graph behind the env step.  The `t` column of the
    monitor rows is passed to the kernels BY VALUE (seconds since `monitor.t_start` when the call is issued): the replays of a
    captured graph repeat the value of the capture.  `monitor_capacity` must be at least the number of envs (all of them can
    finish in one call and two rows must not share a slot)."""

    def __init__(self, env, clip_obs=10.0, clip_reward=10.0, gamma=0.99, eps=1e-8, monitor_capacity=1 << 20, log_dir=None, env_id=""):
        self.env, self.clip_obs, self.clip_reward, self.gamma, self.eps = env, float(clip_obs), float(clip_reward), float(gamma), float(eps)
        self.device = torch.device(env.device)
        self.flat = bool(getattr(env, "flat_observation", False))
        self.obs_dim, self.goal_dim = int(env.obs_dim), 0 if self.flat else int(env.goal_dim)
        self.dim = self.obs_dim + 2 * self.goal_dim
        self.num_envs = E = int(env.num_envs)
        if self.dim > _native.NORM_MAX_DIM:
            raise ValueError("DeviceVecNormalize: observation width %d is above XARM_NORM_MAX_DIM = %d" % (self.dim, _native.NORM_MAX_DIM))
        if int(monitor_capacity) < max(E, 1):
            raise ValueError("DeviceVecNormalize: monitor_capacity %d is below num_envs %d (every env can finish in one call)"
                             % (monitor_capacity, E))
        self.training = True
        self.layout = _native.XarmNormLayout(E, self.obs_dim, self.goal_dim, int(monitor_capacity))
        dev, D = self.device, self.dim
        self.stats = torch.zeros(2 * D + 4, device=dev, dtype=torch.float64)
        self.stats[D:2 * D] = 1.0
        self.stats[2 * D + 1] = 1.0
        self.stats[2 * D + 2:] = 1e-4
        self.ret = torch.zeros(E, device=dev)
        self.monitor = DeviceEpisodeMonitor(E, dev, log_dir, env_id, int(monitor_capacity))
        self._L = self.work = None
        if self.device.type == "cuda":
            self._lib()                               # binds the library and allocates the workspace once, outside any capture

    # ---- the statistics, VecNormalize's names
    @property
    def obs_mean(self):
        return self.stats[:self.dim]

    @property
    def obs_var(self):
        return self.stats[self.dim:2 * self.dim]

    def _lib(self):
        if self._L is None:
            if self.device.type != "cuda":
                raise ValueError("DeviceVecNormalize normalises with HIP kernels on the env's GPU: the env is on '%s'.  There is no "
                                 "host path; train.VecNormalize is the torch implementation." % self.device)
            self._L = _native.load()
            nbytes = C.c_int64(0)
            _native.check(self._L, None, self._L.xarm_norm_work_bytes(C.byref(self.layout), C.byref(nbytes)), "xarm_norm_work_bytes")
            self.work = torch.empty(nbytes.value // 8, device=self.device, dtype=torch.int64)
        return self._L

    def _params(self, t_seconds=0.0):
        return _native.XarmNormParams(self.clip_obs, self.clip_reward, self.eps, self.gamma, t_seconds, 1 if self.training else 0)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _parts(self, obs):
        """the call's three row pointers from the env's observation (dict, or the flat tensor of a 'NoGoal' env)"""
        E = self.num_envs
        parts = [obs] if self.flat else [obs["observation"], obs["achieved_goal"], obs["desired_goal"]]
        for x, w in zip(parts, (self.obs_dim, self.goal_dim, self.goal_dim)):
            assert x.dtype == torch.float32 and x.is_contiguous() and x.shape == (E, w) and x.device == self.stats.device, \
                "observation parts must be contiguous float32 [num_envs, dim] tensors on the env's device"
        return [C.c_void_p(x.data_ptr()) for x in parts] + [None] * (3 - len(parts))

    def _u8(self, x, what):
        if x.dtype == torch.bool:
            x = x.view(torch.uint8)                  # same bytes, no copy
        assert x.dtype == torch.uint8 and x.is_contiguous() and x.shape == (self.num_envs,) and x.device == self.stats.device, what
        return C.c_void_p(x.data_ptr())

    def alloc_out(self):
        """the tensors step_into fills"""
        return {"nobs": torch.empty(self.num_envs, self.dim, device=self.device), "nrew": torch.empty(self.num_envs, device=self.device)}

    def reset(self):
        self._lib()                                   # a CPU env is refused before it is touched
        return self.reset_from(self.env.reset())

    def reset_from(self, obs):
        """reset()'s work on an observation the caller took from env.reset() itself (gym_xarm_amd/sac.py keeps the raw dict for its
        replay buffer): the returns are zeroed, the statistics updated and the normalised observation returned"""
        L = self._lib()
        nobs = torch.empty(self.num_envs, self.dim, device=self.device)
        rc = L.xarm_norm_obs(C.byref(self.layout), C.byref(self._params()), C.c_void_p(self.stats.data_ptr()),
                             C.c_void_p(self.ret.data_ptr()), C.c_void_p(self.work.data_ptr()), *self._parts(obs), 1,
                             C.c_void_p(nobs.data_ptr()), self._stream())
        _native.check(L, None, rc, "xarm_norm_obs")
        return nobs

    def normalize_rows(self, out, observation, achieved_goal=None, desired_goal=None):
        """out [B, dim] <- the B rows observation | achieved_goal | desired_goal normalised with the statistics as they are (one
        xarm_norm_obs launch with update = 0; nothing is updated).  B is free: the rows of a replay sample.  The call's workspace is
        allocated at the first call with a given B; after that no allocation and no host read, so it can be captured."""
        L = self._lib()
        B = int(observation.shape[0])
        parts = [observation] if self.goal_dim == 0 else [observation, achieved_goal, desired_goal]
        for x, w in zip(parts, (self.obs_dim, self.goal_dim, self.goal_dim)):
            assert x.dtype == torch.float32 and x.is_contiguous() and x.shape == (B, w) and x.device == self.stats.device, \
                "row parts must be contiguous float32 [B, dim] tensors on the env's device"
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == (B, self.dim) and out.device == self.stats.device, "out"
        if not hasattr(self, "_row_calls"):
            self._row_calls = {}
        if B not in self._row_calls:
            layout = _native.XarmNormLayout(B, self.obs_dim, self.goal_dim, max(B, 1))
            nbytes = C.c_int64(0)
            _native.check(L, None, L.xarm_norm_work_bytes(C.byref(layout), C.byref(nbytes)), "xarm_norm_work_bytes")
            self._row_calls[B] = (layout, torch.empty(max(nbytes.value // 8, 1), device=self.device, dtype=torch.int64))
        layout, work = self._row_calls[B]
        params = _native.XarmNormParams(self.clip_obs, self.clip_reward, self.eps, self.gamma, 0.0, 0)
        rc = L.xarm_norm_obs(C.byref(layout), C.byref(params), C.c_void_p(self.stats.data_ptr()), None, C.c_void_p(work.data_ptr()),
                             *([C.c_void_p(x.data_ptr()) for x in parts] + [None] * (3 - len(parts))), 0, C.c_void_p(out.data_ptr()), self._stream())
        _native.check(L, None, rc, "xarm_norm_obs")
        return out

    def step_into(self, out, obs, rew, done, keep=None, t_seconds=None):
        """Normalise one env step's outputs into out["nobs"] [E, dim] / out["nrew"] [E] and update statistics, returns and the
        monitor in place.  obs: the env's dict (or flat tensor), rew float32 [E], done uint8 / bool [E], keep: uint8 / bool [E]
        rows that are real transitions, or None.  No allocation, no host read; capturable (t_seconds is captured by value)."""
        L, m, p = self._lib(), self.monitor, lambda t: C.c_void_p(t.data_ptr())
        E = self.num_envs
        assert rew.dtype == torch.float32 and rew.is_contiguous() and rew.shape == (E,) and rew.device == self.stats.device, "rew"
        for k, shape in (("nobs", (E, self.dim)), ("nrew", (E,))):
            assert out[k].dtype == torch.float32 and out[k].is_contiguous() and out[k].shape == shape and out[k].device == self.stats.device, k
        t = time.time() - m.t_start if t_seconds is None else t_seconds
        rc = L.xarm_norm_step(C.byref(self.layout), C.byref(self._params(t)), p(self.stats), p(self.ret), p(m.ep_ret), p(m.ep_len),
                              p(m.ring), p(m.n_dev), p(self.work), *self._parts(obs), p(rew), self._u8(done, "done"),
                              None if keep is None else self._u8(keep, "keep"), p(out["nobs"]), p(out["nrew"]), self._stream())
        _native.check(L, None, rc, "xarm_norm_step")
        return out

    def step(self, actions):
        obs, rew, done, info = self.env.step(actions)
        # lazy auto-reset: rows spending this call on a reset tick stay out of the statistics and the episode sums; the mask
        # goes to the kernels as it is, the host never reads it
        keep = ~info["resetting"] if "resetting" in info else None
        out = self.step_into(self.alloc_out(), obs, rew, done, keep)
        return out["nobs"], out["nrew"], done, info, rew

    def state_dict(self):
        s, D = self.stats.detach().cpu(), self.dim
        f32 = lambda x: x.to(torch.float32).clone()
        return {"obs_mean": f32(s[:D]), "obs_var": f32(s[D:2 * D]), "obs_count": s[2 * D + 2].clone(),
                "ret_mean": f32(s[2 * D]), "ret_var": f32(s[2 * D + 1]), "ret_count": s[2 * D + 3].clone(),
                "clip_obs": torch.tensor(float(self.clip_obs)), "clip_reward": torch.tensor(float(self.clip_reward)),
                "gamma": torch.tensor(float(self.gamma)),
                "obs_mean_f64": s[:D].clone(), "obs_var_f64": s[D:2 * D].clone(), "ret_mean_f64": s[2 * D].clone(),
                "ret_var_f64": s[2 * D + 1].clone()}

    def load_state_dict(self, sd):
        D = self.dim
        if tuple(sd["obs_mean"].shape) != (D,):
            raise ValueError("VecNormalize statistics are for observation width %d, this env has %d" % (sd["obs_mean"].shape[0], D))
        pick = lambda k: (sd[k + "_f64"] if k + "_f64" in sd else sd[k]).detach().to("cpu", torch.float64)
        s = self.stats.detach().cpu()
        s[:D], s[D:2 * D], s[2 * D + 2] = pick("obs_mean"), pick("obs_var"), float(sd["obs_count"])
        if "ret_mean" in sd:      # as VecNormalize: older files hold the observation statistics only
            s[2 * D], s[2 * D + 1], s[2 * D + 3] = pick("ret_mean"), pick("ret_var"), float(sd["ret_count"])
        self.stats.copy_(s)
        self.clip_obs = float(sd["clip_obs"]) if "clip_obs" in sd else self.clip_obs
        self.clip_reward = float(sd["clip_reward"]) if "clip_reward" in sd else self.clip_reward
        self.gamma = float(sd["gamma"]) if "gamma" in sd else self.gamma

    def save(self, path):
        """VecNormalize.save's file, plus the *_f64 keys"""
        from safetensors.torch import save_file
        save_file({k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, env, **kw):
        from safetensors.torch import load_file
        v = cls(env, **kw)
        v.load_state_dict(load_file(path))
        return v
