"""Uniform replay buffer for the batched envs, resident on the env's device: stable-baselines3's plain `ReplayBuffer`.

The reference's deployment script loads a SAC agent for the flat Handover env (`benchmark/display.py`: `SAC.load("sac_hanover")`, a
29-wide observation in its `vec_normalize.pkl`): an agent trained on SB3's `ReplayBuffer`, not on HER.  This is that buffer.  Every
stored transition - of running episodes too - is sampled with the same probability and nothing is relabelled, so it serves a
flat-observation env (`XarmPDHandoverNoGoal-v1`) and a goal env with a dense reward alike; on a goal env a row is
observation | achieved_goal | desired_goal, the learner's flat observation.  As SB3's buffer does with
`handle_timeout_termination=True`, a sample's `done` is `done and not timeout`: the TD target bootstraps through a time-limit
truncation (`info["TimeLimit.truncated"]`).  The HER buffers (gym_xarm_amd/her.py) still store truncations as terminations.

`ReplayBuffer` is the buffer in torch ops, the default on a CPU env and the checker; `DeviceReplayBuffer` keeps one ring of records
and runs `add` / `sample` in HIP kernels (csrc/xarm_k_replay.hip): O(E) per add, and one launch writes the batch
as the device learners take it - both observation rows normalised, done as float, use - with no host read and no allocation.
"""
import torch


def _row(obs, nxt=None):
    """the flat observation row of `obs` (tensor, or the env's dict); with `nxt` the next row: its observation and achieved goal with
    `obs`'s desired goal"""
    if torch.is_tensor(obs):
        return obs if nxt is None else nxt
    if nxt is None:
        return torch.cat([obs["observation"], obs["achieved_goal"], obs["desired_goal"]], dim=1)
    return torch.cat([nxt["observation"], nxt["achieved_goal"], obs["desired_goal"]], dim=1)


def _dims(env):
    flat = bool(getattr(env, "flat_observation", False))
    obs_dim, goal_dim = int(env.obs_dim), 0 if flat else int(env.goal_dim)
    return obs_dim, goal_dim, int(getattr(env, "action_dim", getattr(env, "act_dim", 0)))


class ReplayBuffer:
    """SB3's `ReplayBuffer` on the env's device: horizon = max(buffer_size // num_envs, 1) slots per env, sampled uniformly over
    the filled slots times the envs."""

    def __init__(self, env, buffer_size=1_000_000, handle_timeout_termination=True, seed=0):
        self.E, self.device = int(env.num_envs), torch.device(env.device)
        self.obs_dim, self.goal_dim, self.act_dim = _dims(env)
        self.dim = self.obs_dim + 2 * self.goal_dim
        self.horizon = max(int(buffer_size) // max(self.E, 1), 1)
        self.handle_timeout_termination = bool(handle_timeout_termination)
        T, E, dev = self.horizon, self.E, self.device
        f = dict(device=dev, dtype=torch.float32)
        self.obs, self.next_obs = torch.zeros(T, E, self.dim, **f), torch.zeros(T, E, self.dim, **f)
        self.act = torch.zeros(T, E, self.act_dim, **f)
        self.rew = torch.zeros(T, E, **f)
        self.done = torch.zeros(T, E, device=dev, dtype=torch.bool)
        self.timeout = torch.zeros(T, E, device=dev, dtype=torch.bool)
        self.t = 0
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)

    def add(self, obs, next_obs, action, reward, done, timeout=None):
        """One transition per env.  obs / next_obs: the flat tensor [E, D], or the env's dicts (next_obs needs "observation" and
        "achieved_goal"; the desired goal is obs's).  For envs with `done` set pass the terminal observation as next_obs.
        timeout: bool [E], the envs whose done is a time-limit truncation (info["TimeLimit.truncated"]); None: none."""
        s = self.t % self.horizon
        self.obs[s], self.next_obs[s] = _row(obs), _row(obs, next_obs)
        self.act[s], self.rew[s] = action, reward
        self.done[s] = torch.as_tensor(done, device=self.device) != 0
        self.timeout[s] = False if timeout is None else (torch.as_tensor(timeout, device=self.device) != 0)
        self.t += 1

    def filled(self):
        return min(self.t, self.horizon)

    def sample(self, batch_size, index=None):
        """-> {"obs", "next_obs" [B, D] (raw), "action" [B, A], "reward" [B], "done" [B] float (time-limit truncations taken out when
        handle_timeout_termination), "use" [B] float, "env", "time" [B] int64}.  index = (slots, envs): these picks instead of a draw.
        While the buffer is empty every row is zero with use = 0."""
        B, dev = int(batch_size), self.device
        n = self.filled() * self.E
        if n == 0:
            f = dict(device=dev, dtype=torch.float32)
            z = torch.zeros(B, dtype=torch.int64, device=dev)
            return {"obs": torch.zeros(B, self.dim, **f), "next_obs": torch.zeros(B, self.dim, **f), "action": torch.zeros(B, self.act_dim, **f),
                    "reward": torch.zeros(B, **f), "done": torch.zeros(B, **f), "use": torch.zeros(B, **f), "env": z, "time": z.clone()}
        if index is None:
            pick = torch.randint(n, (B,), device=dev, generator=self.gen)
            s, e = pick // self.E, pick % self.E
        else:
            s, e = (torch.as_tensor(x, device=dev).to(torch.int64) for x in index)
        done = self.done[s, e]
        if self.handle_timeout_termination:
            done = done & ~self.timeout[s, e]
        last = self.t - 1
        return {"obs": self.obs[s, e], "next_obs": self.next_obs[s, e], "action": self.act[s, e], "reward": self.rew[s, e],
                "done": done.to(torch.float32), "use": torch.ones(B, device=dev), "env": e, "time": last - (last - s) % self.horizon}


class DeviceReplayBuffer:
    """ReplayBuffer with its storage and sampling in HIP kernels (csrc/xarm_k_replay.hip).

    One float32 ring [horizon, E, R] holds a record obs | next_obs | action | reward | done | timeout per (slot, env), R = 2 D + A + 3;
    `add` is one launch plus the clock tick, `sample_into` one launch plus the tick: row b takes the entry
    mulhi64(Philox(seed; b, sample_calls), min(t, horizon) E) - no rejection, no atomics, no host read, no allocation, so it can be
    captured in a torch.cuda.graph (the clock {t, sample_calls} lives on the device and each replay draws a fresh batch).  Same
    constructor and `add` as ReplayBuffer; `sample` returns its dict."""

    OUT_KEYS = ("obs", "next_obs", "action", "reward", "done", "use", "env", "time")

    def __init__(self, env, buffer_size=1_000_000, handle_timeout_termination=True, seed=0):
        import ctypes as C
        from . import _native
        self.E, self.device = int(env.num_envs), torch.device(env.device)
        if self.device.type != "cuda":
            raise ValueError("DeviceReplayBuffer keeps its ring on the GPU and samples it with HIP kernels: the env is on "
                             "'%s'.  There is no host path; ReplayBuffer is the torch implementation." % self.device)
        self.obs_dim, self.goal_dim, self.act_dim = _dims(env)
        self.dim = self.obs_dim + 2 * self.goal_dim
        self.horizon = max(int(buffer_size) // max(self.E, 1), 1)
        self.handle_timeout_termination, self.seed = bool(handle_timeout_termination), int(seed)
        self._C, self._L, self._check = C, _native.load(), _native.check
        self.layout = _native.XarmReplayLayout(self.E, self.horizon, self.obs_dim, self.goal_dim, self.act_dim)
        self.record_floats = self._L.xarm_replay_record_floats(C.byref(self.layout))
        if self.record_floats < 0:
            self._check(self._L, None, self.record_floats, "xarm_replay_record_floats")
        self.ring = torch.zeros(self.horizon, self.E, self.record_floats, device=self.device, dtype=torch.float32)
        self.clock = torch.zeros(2, device=self.device, dtype=torch.int64)        # {t, sample_calls}

    def _p(self, t):
        return None if t is None else self._C.c_void_p(t.data_ptr())

    def _stream(self):
        return self._C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _rows(self, x, dim):
        x = torch.as_tensor(x, device=self.device)
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        assert x.shape == ((self.E, dim) if dim else (self.E,)), (tuple(x.shape), dim)
        return x

    def _u8(self, x):
        x = torch.as_tensor(x, device=self.device)
        if x.dtype == torch.bool and x.is_contiguous():
            x = x.view(torch.uint8)                  # same bytes, no copy
        x = x if x.dtype == torch.uint8 and x.is_contiguous() else (x != 0).to(torch.uint8).contiguous()
        assert x.shape == (self.E,)
        return x

    def add(self, obs, next_obs, action, reward, done, timeout=None):
        """One transition per env, ReplayBuffer.add's arguments.  Float32 contiguous device tensors are read in place."""
        if self.goal_dim == 0:
            assert torch.is_tensor(obs) and torch.is_tensor(next_obs), "a flat-observation buffer takes the observation tensors"
            parts = [self._rows(obs, self.obs_dim), None, None, self._rows(next_obs, self.obs_dim), None]
        else:
            parts = [self._rows(obs["observation"], self.obs_dim), self._rows(obs["achieved_goal"], self.goal_dim),
                     self._rows(obs["desired_goal"], self.goal_dim), self._rows(next_obs["observation"], self.obs_dim),
                     self._rows(next_obs["achieved_goal"], self.goal_dim)]
        rest = [self._rows(action, self.act_dim), self._rows(reward, 0), self._u8(done), None if timeout is None else self._u8(timeout)]
        rc = self._L.xarm_replay_add(self._C.byref(self.layout), self._p(self.ring), self._p(self.clock), *[self._p(x) for x in parts + rest],
                                     self._stream())
        self._check(self._L, None, rc, "xarm_replay_add")

    @property
    def t(self):
        """transitions stored per env so far (reads the device clock: a host sync)"""
        return int(self.clock[0].item())

    def alloc_out(self, batch_size):
        """the [B, .] tensors sample_into fills"""
        B, f = int(batch_size), dict(device=self.device, dtype=torch.float32)
        i = dict(device=self.device, dtype=torch.int64)
        return {"obs": torch.empty(B, self.dim, **f), "next_obs": torch.empty(B, self.dim, **f), "action": torch.empty(B, self.act_dim, **f),
                "reward": torch.empty(B, **f), "done": torch.empty(B, **f), "use": torch.empty(B, **f), "env": torch.empty(B, **i),
                "time": torch.empty(B, **i)}

    def sample_into(self, out, normalize=None):
        """Fill the preallocated contiguous tensors of `out` (alloc_out's keys and dtypes, B = rows of out["reward"]; "env" and "time"
        may be left out): the sample kernel and the clock tick on the current stream.  normalize: a DeviceVecNormalize whose
        statistics - as they are, nothing is updated - normalise "obs" and "next_obs" inside the kernel; None: the rows are copied.
        No allocation, no host sync; capturable."""
        B = int(out["reward"].shape[0])
        for k, dt, w in (("obs", torch.float32, self.dim), ("next_obs", torch.float32, self.dim), ("action", torch.float32, self.act_dim),
                         ("reward", torch.float32, 0), ("done", torch.float32, 0), ("use", torch.float32, 0), ("env", torch.int64, 0),
                         ("time", torch.int64, 0)):
            if k in ("env", "time") and out.get(k) is None:
                continue
            x = out[k]
            assert x.dtype == dt and x.is_contiguous() and tuple(x.shape) == ((B, w) if w else (B,)) and x.device == self.ring.device, k
        stats, clip_obs, eps = None, 1.0, 1.0
        if normalize is not None:
            if int(normalize.dim) != self.dim:
                raise ValueError("DeviceReplayBuffer: the normaliser's statistics are for observation width %d, the buffer's rows have %d"
                                 % (int(normalize.dim), self.dim))
            stats, clip_obs, eps = normalize.stats, float(normalize.clip_obs), float(normalize.eps)
            assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.device == self.ring.device, "normalize.stats"
        rc = self._L.xarm_replay_sample(self._C.byref(self.layout), self._p(self.ring), self._p(self.clock), self.seed, B,
                                        int(self.handle_timeout_termination), self._p(stats), clip_obs, eps,
                                        *[self._p(out.get(k)) for k in self.OUT_KEYS], self._stream())
        self._check(self._L, None, rc, "xarm_replay_sample")
        return out

    def sample(self, batch_size, normalize=None):
        """ReplayBuffer.sample's dict (allocates)"""
        return self.sample_into(self.alloc_out(batch_size), normalize)


UNIFORM_BUFFERS = (ReplayBuffer, DeviceReplayBuffer)
