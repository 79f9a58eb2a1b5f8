"""Hindsight-experience-replay buffer for the batched goal envs, resident on the env's device.

The reference's training script asks SB3 for `HerReplayBuffer(n_sampled_goal=4, goal_selection_strategy="future",
online_sampling=True)` (benchmark/train.py:82-97); what that buffer needs from the env is exactly the batched
`compute_reward(achieved_goal, goal, info)` of the GoalEnv API (xarm_pick_and_place.py:155-177, xarm_reach.py:107-116,
xarm_handover.py:153-183).  Here the transitions of all E envs are stored time-major as device tensors and a
sampled batch is relabelled with one gather + one `compute_reward` kernel launch (the C-ABI's `xarm_compute_reward`),
no host round trip.

Layout: a ring of `horizon` time slots, each holding one transition per env.  `ep_end[slot, env]` is the absolute
time of the last transition of the episode the entry belongs to, or -1 while that episode is still running; only
entries of finished episodes are sampled ("future" needs the episode's end).

`HerReplayBuffer` is that buffer in torch ops; `DeviceHerReplayBuffer` is the same buffer with one ring of records and its
`add` / `sample` in HIP kernels (csrc/xarm_k_her.hip): O(E) per add, no host read and no allocation per sample.
"""
import torch


class HerReplayBuffer:
    def __init__(self, env, horizon=None, n_sampled_goal=4, goal_selection_strategy="future", reward_fn=None, seed=0):
        assert goal_selection_strategy in ("future", "final"), goal_selection_strategy
        self.E, self.device = env.num_envs, env.device
        max_len = int(getattr(env, "max_episode_steps", 50))
        self.horizon = int(horizon) if horizon else 4 * max_len
        assert self.horizon >= 2 * max_len, "the ring must hold at least two full episodes per env"
        self.strategy = goal_selection_strategy
        self.her_ratio = 1.0 - 1.0 / (n_sampled_goal + 1)          # SB3: n_sampled_goal virtual per real transition
        self.reward_fn = reward_fn if reward_fn is not None else env.compute_reward
        T, E, dev = self.horizon, self.E, self.device
        f = dict(device=dev, dtype=torch.float32)
        self.obs = torch.zeros(T, E, env.obs_dim, **f)
        self.next_obs = torch.zeros(T, E, env.obs_dim, **f)
        self.ag = torch.zeros(T, E, env.goal_dim, **f)
        self.next_ag = torch.zeros(T, E, env.goal_dim, **f)
        self.dg = torch.zeros(T, E, env.goal_dim, **f)
        self.act = torch.zeros(T, E, env.action_dim, **f)
        self.rew = torch.zeros(T, E, **f)
        self.done = torch.zeros(T, E, device=dev, dtype=torch.bool)
        self.ep_end = torch.full((T, E), -1, device=dev, dtype=torch.int64)
        self.slot_time = torch.full((T,), -1, device=dev, dtype=torch.int64)   # absolute time stored in each slot
        self.ep_start = torch.zeros(E, device=dev, dtype=torch.int64)          # absolute time each env's episode began
        self.t = 0
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)

    def add(self, obs, next_obs, action, reward, done):
        """One transition per env.  `obs` / `next_obs` are the env's dicts; for envs with `done` set pass the
        terminal observation (info["terminal_observation"]) as `next_obs`, not the post-reset one."""
        s = self.t % self.horizon
        self.obs[s], self.next_obs[s] = obs["observation"], next_obs["observation"]
        self.ag[s], self.next_ag[s], self.dg[s] = obs["achieved_goal"], next_obs["achieved_goal"], obs["desired_goal"]
        self.act[s], self.rew[s] = action, reward
        d = done.to(torch.bool)
        self.done[s] = d
        self.ep_end[s] = -1
        self.slot_time[s] = self.t
        # close the episodes that ended now: every stored entry of env e with ep_start[e] <= time <= t
        inside = (self.slot_time[:, None] >= self.ep_start[None, :]) & d[None, :]
        self.ep_end = torch.where(inside, torch.full_like(self.ep_end, self.t), self.ep_end)
        self.ep_start = torch.where(d, torch.full_like(self.ep_start, self.t + 1), self.ep_start)
        self.t += 1

    def num_valid(self):
        return int(self._valid().sum().item())

    def _valid(self):
        # finished episodes whose first entry has not been overwritten since
        return (self.ep_end >= 0) & (self.slot_time[:, None] > self.t - 1 - self.horizon)

    def sample(self, batch_size):
        """-> dict of [B, .] tensors; the first round(her_ratio * B) rows carry a relabelled goal and a recomputed
        reward, the rest are the stored transitions."""
        valid = self._valid().flatten().nonzero().squeeze(1)
        if valid.numel() == 0:
            raise RuntimeError("HerReplayBuffer.sample: no finished episode stored yet")
        pick = valid[torch.randint(valid.numel(), (batch_size,), device=self.device, generator=self.gen)]
        s, e = pick // self.E, pick % self.E
        t_abs, end = self.slot_time[s], self.ep_end[s, e]
        n_her = int(round(self.her_ratio * batch_size))
        if self.strategy == "future":
            u = torch.rand(batch_size, device=self.device, generator=self.gen)
            t_goal = t_abs + (u * (end - t_abs + 1).to(torch.float32)).to(torch.int64)
            t_goal = torch.minimum(t_goal, end)
        else:
            t_goal = end
        new_goal = self.next_ag[t_goal % self.horizon, e]
        goal = self.dg[s, e].clone()
        goal[:n_her] = new_goal[:n_her]
        next_ag = self.next_ag[s, e]
        reward = self.rew[s, e].clone()
        if n_her > 0:
            reward[:n_her] = self.reward_fn(next_ag[:n_her].contiguous(), goal[:n_her].contiguous(), None)
        return {"observation": self.obs[s, e], "next_observation": self.next_obs[s, e], "achieved_goal": self.ag[s, e],
                "next_achieved_goal": next_ag, "desired_goal": goal, "action": self.act[s, e], "reward": reward,
                "done": self.done[s, e], "relabelled": torch.arange(batch_size, device=self.device) < n_her,
                "env": e, "time": t_abs, "goal_time": t_goal}


class DeviceHerReplayBuffer:
    """HerReplayBuffer with its storage, bookkeeping and sampling in HIP kernels (csrc/xarm_k_her.hip).

    One float32 ring [horizon, E, R] holds a record per (slot, env); `add` costs O(E) plus O(episode length) for the envs that
    finished, `sample_into` is rejection sampling on the device: no list of valid entries, no host read, no allocation, so it
    can be captured in a torch.cuda.graph (the clock {t, sample_calls} lives on the device and each replay advances it).
    Same constructor, `add` and `sample` as HerReplayBuffer; additionally the strategy 'episode' (SB3's: a goal from anywhere
    in the episode) and, per row, "ok": a row is False and all zero when 64 uniform proposals all hit running episodes -
    probability (1 - v)^64 at a valid share v of the stored entries, < 1e-8 once a quarter of them is valid."""

    OUT_KEYS = ("observation", "next_observation", "achieved_goal", "next_achieved_goal", "desired_goal", "action", "reward",
                "done", "env", "time", "goal_time", "ok")

    def __init__(self, env, horizon=None, n_sampled_goal=4, goal_selection_strategy="future", reward_fn=None, seed=0):
        import ctypes as C
        from . import _native
        assert goal_selection_strategy in _native.HER_STRATEGIES, goal_selection_strategy
        self.E, self.device = env.num_envs, torch.device(env.device)
        if self.device.type != "cuda":
            raise ValueError("DeviceHerReplayBuffer keeps its ring on the GPU and samples it with HIP kernels: the env is on "
                             "'%s'.  There is no host path; HerReplayBuffer is the torch implementation." % self.device)
        max_len = int(getattr(env, "max_episode_steps", 50))
        self.horizon = int(horizon) if horizon else 4 * max_len
        assert self.horizon >= 2 * max_len, "the ring must hold at least two full episodes per env"
        self.strategy = goal_selection_strategy
        self.her_ratio = 1.0 - 1.0 / (n_sampled_goal + 1)
        self.env, self.reward_fn, self.seed = env, reward_fn, int(seed)
        self.obs_dim, self.goal_dim, self.act_dim = int(env.obs_dim), int(env.goal_dim), int(env.action_dim)
        self._C, self._L = C, _native.load()
        self._check = _native.check
        self._strategy_id = _native.HER_STRATEGIES[goal_selection_strategy]
        self.layout = _native.XarmHerLayout(self.E, self.horizon, self.obs_dim, self.goal_dim, self.act_dim)
        self.record_floats = self._L.xarm_her_record_floats(C.byref(self.layout))
        if self.record_floats < 0:
            self._check(self._L, None, self.record_floats, "xarm_her_record_floats")
        T, E, dev = self.horizon, self.E, self.device
        self.ring = torch.zeros(T, E, self.record_floats, device=dev, dtype=torch.float32)
        self.ep_end = torch.full((T, E), -1, device=dev, dtype=torch.int64)
        self.ep_first = torch.full((T, E), -1, device=dev, dtype=torch.int64)
        self.ep_start = torch.zeros(E, device=dev, dtype=torch.int64)
        self.clock = torch.zeros(2, device=dev, dtype=torch.int64)        # {t, sample_calls}
        self.fail_count = torch.zeros(1, device=dev, dtype=torch.int64)   # rows that ran out of proposals, over all calls

    def _p(self, t):
        return self._C.c_void_p(t.data_ptr())

    def _stream(self):
        return self._C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _rows(self, x, dim):
        x = torch.as_tensor(x, device=self.device)
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.to(torch.float32).contiguous()
        assert x.shape == ((self.E, dim) if dim else (self.E,)), (tuple(x.shape), dim)
        return x

    def add(self, obs, next_obs, action, reward, done):
        """One transition per env, HerReplayBuffer.add's arguments.  Float32 contiguous device tensors are read in place."""
        d = torch.as_tensor(done, device=self.device)
        d = d if d.dtype == torch.uint8 and d.is_contiguous() else (d != 0).to(torch.uint8).contiguous()
        assert d.shape == (self.E,)
        a = [self._rows(obs["observation"], self.obs_dim), self._rows(next_obs["observation"], self.obs_dim),
             self._rows(obs["achieved_goal"], self.goal_dim), self._rows(next_obs["achieved_goal"], self.goal_dim),
             self._rows(obs["desired_goal"], self.goal_dim), self._rows(action, self.act_dim), self._rows(reward, 0), d]
        rc = self._L.xarm_her_add(self._C.byref(self.layout), self._p(self.ring), self._p(self.ep_end), self._p(self.ep_first),
                                  self._p(self.ep_start), self._p(self.clock), *[self._p(x) for x in a], self._stream())
        self._check(self._L, None, rc, "xarm_her_add")

    @property
    def t(self):
        """transitions stored per env so far (reads the device clock: a host sync)"""
        return int(self.clock[0].item())

    def num_valid(self):
        return int((self.ep_end >= 0).sum().item())

    def n_her(self, batch_size):
        return int(round(self.her_ratio * batch_size))

    def alloc_out(self, batch_size):
        """the [B, .] tensors sample_into fills"""
        B, f = int(batch_size), dict(device=self.device, dtype=torch.float32)
        i = dict(device=self.device, dtype=torch.int64)
        return {"observation": torch.empty(B, self.obs_dim, **f), "next_observation": torch.empty(B, self.obs_dim, **f),
                "achieved_goal": torch.empty(B, self.goal_dim, **f), "next_achieved_goal": torch.empty(B, self.goal_dim, **f),
                "desired_goal": torch.empty(B, self.goal_dim, **f), "action": torch.empty(B, self.act_dim, **f),
                "reward": torch.empty(B, **f), "done": torch.empty(B, device=self.device, dtype=torch.bool),
                "env": torch.empty(B, **i), "time": torch.empty(B, **i), "goal_time": torch.empty(B, **i),
                "ok": torch.empty(B, device=self.device, dtype=torch.bool)}

    def sample_into(self, out):
        """Fill the preallocated contiguous tensors of `out` (alloc_out's keys and dtypes; B = rows of out["reward"]): the
        sample kernel, the clock tick, the env's reward kernel on rows [0, n_her) and one in-place multiply of those rewards by
        their ok flags, on the current stream.  No allocation, no host sync; capturable.  (A custom reward_fn is called instead
        of the reward kernel and may allocate.)"""
        B = int(out["reward"].shape[0])
        n_her = self.n_her(B)
        for k in self.OUT_KEYS:
            assert out[k].is_contiguous() and out[k].shape[0] == B and out[k].device == self.ring.device, k
        rc = self._L.xarm_her_sample(self._C.byref(self.layout), self._p(self.ring), self._p(self.ep_end), self._p(self.ep_first),
                                     self._p(self.clock), self.seed, self._strategy_id, B, n_her,
                                     *[self._p(out[k]) for k in self.OUT_KEYS[:-1]], self._p(out["ok"]), self._p(self.fail_count),
                                     self._stream())
        self._check(self._L, None, rc, "xarm_her_sample")
        if n_her > 0:
            if self.reward_fn is not None:
                out["reward"][:n_her] = self.reward_fn(out["next_achieved_goal"][:n_her], out["desired_goal"][:n_her], None)
            else:   # relabelled rows come first: [0, n_her) of next_achieved_goal / desired_goal / reward are contiguous
                env = self.env
                rc = env._L.xarm_compute_reward(env._h, self._p(out["next_achieved_goal"]), self._p(out["desired_goal"]), n_her,
                                                self._p(out["reward"]), self._stream())
                self._check(env._L, env._h, rc, "xarm_compute_reward")
            # a failed row is all zero, its reward included: compute_reward(0, 0) is a success under the sparse rewards
            torch.mul(out["reward"][:n_her], out["ok"][:n_her], out=out["reward"][:n_her])
        return out

    def sample(self, batch_size):
        """HerReplayBuffer.sample's dict plus "ok"; reads the ok flags back once (the only host sync of this class's sampling)
        to raise HerReplayBuffer's error when no row found a finished episode."""
        out = self.sample_into(self.alloc_out(batch_size))
        if batch_size > 0 and not bool(out["ok"].any().item()):
            raise RuntimeError("HerReplayBuffer.sample: no finished episode stored yet")
        out["relabelled"] = torch.arange(int(batch_size), device=self.device) < self.n_her(batch_size)
        return out


def collect(env, buffer, policy, steps, obs=None):
    """Roll `steps` env steps with policy(obs_dict) -> actions[E, A] and store them.  The env's tensors are reused
    from step to step, so the previous observation is cloned before stepping, and finished envs contribute their
    terminal observation (info['terminal_observation']) instead of the post-reset one."""
    assert not getattr(env, "_lazy", False), "HER collection assumes the reference's in-call auto-reset (auto_reset=True)"
    if obs is None:
        obs = env.reset()
    for _ in range(steps):
        prev = {k: v.clone() for k, v in obs.items()}
        act = policy(prev)
        obs, rew, done, info = env.step(act)
        d = (done != 0)[:, None]
        term = info["terminal_observation"]
        nxt = {"observation": torch.where(d, term, obs["observation"]),
               "achieved_goal": torch.where(d, env.achieved_goal_of(term), obs["achieved_goal"])}
        buffer.add(prev, nxt, act, rew, done)
    return obs
