"""ctypes view of tests/hostbuild_eval (g++ build of csrc/xarm_eval_core.h) - CPU-side evaluation tests only - the scripted streams the
host and GPU evaluation tests share, and a plain-Python restatement of the semantics the streams are checked against."""
import ctypes as C
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "hostbuild_eval")
GXX_FLAGS = ["-O1", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]       # tests/replay_host.py's
SHAPES = ((1, 1), (1, 5), (3, 2), (3, 7), (64, 64), (65, 100), (130, 131), (257, 300))      # (E, N)
THREADS = 256            # csrc/xarm_eval_core.h THREADS
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "libeval_host.so")
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    srcs = [os.path.join(DIR, "eval_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + [
        os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + GXX_FLAGS + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.eh_begin.argtypes = [vp] * 6
    L.eh_step.argtypes = [vp] * 10
    L.eh_summary.argtypes = [vp] * 4
    L.eh_target.argtypes = [vp, C.c_int32]
    L.eh_base.argtypes = [vp, C.c_int32]
    _lib = L
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class HostEval:
    """the evaluation state of csrc/xarm_eval_core.h on NumPy arrays"""

    STATE = ("cur_ret", "cur_len", "count", "remaining", "records")

    def __init__(self, E, N):
        from gym_xarm_amd import _native
        self.E, self.N = E, N
        self.layout = _native.XarmEvalLayout(E, N)
        self.cur_ret, self.cur_len, self.count = np.full(E, 7.0), np.full(E, 7, np.int32), np.full(E, 7, np.int32)   # 7: begin must write it
        self.remaining, self.records, self.out = np.full(1, 7, np.int32), np.full((N, 3), 7.0), np.full(8, 7.0)

    def _state(self):
        return [_p(getattr(self, k)) for k in self.STATE]

    def begin(self):
        assert lib().eh_begin(C.byref(self.layout), *self._state()) == 0

    def step(self, rew, done, success, keep=None):
        assert lib().eh_step(C.byref(self.layout), *self._state(), _p(rew), _p(done), _p(success), _p(keep)) == 0

    def summary(self):
        assert lib().eh_summary(C.byref(self.layout), _p(self.count), _p(self.records), _p(self.out)) == 0
        return self.out

    def state(self):
        return {k: getattr(self, k).copy() for k in self.STATE}


# ---- the scripted streams
def ep_lens(E):
    """per-env episode lengths in the style of replay_host.ep_lens, one env of length 1"""
    return [(3, 4, 5, 5, 2, 4, 1)[e % 7] for e in range(E)]


def reward(e, t):
    """exactly representable (multiples of 1/4), so that every float64 sum is exact; its std is above its mean's magnitude"""
    return (e % 8) / 4.0 - (t % 5) * 0.5 + 0.25


def success(e, t):
    return (e + t) % 3 == 0


def kept(e, t):
    return (e * 7 + t) % 4 != 0


class Stream:
    """step t of the scripted stream: rew float32 [E], done / success uint8 [E], keep uint8 [E] or None.  An env's episode ends after
    ep_lens[e] KEPT steps; a masked step is never done (as a lazy-reset tick is not)."""

    def __init__(self, E, use_keep=False):
        self.E, self.use_keep, self.t = E, use_keep, 0
        self.lens, self.steps = ep_lens(E), [0] * E

    def next(self):
        E, t = self.E, self.t
        keep = [1 if (not self.use_keep or kept(e, t)) else 0 for e in range(E)]
        done = [0] * E
        for e in range(E):
            self.steps[e] += keep[e]
            if keep[e] and self.steps[e] >= self.lens[e]:
                done[e], self.steps[e] = 1, 0
        rew = np.array([reward(e, t) for e in range(E)], np.float32)
        succ = np.array([1 if success(e, t) else 0 for e in range(E)], np.uint8)
        self.t += 1
        return rew, np.array(done, np.uint8), succ, (np.array(keep, np.uint8) if self.use_keep else None)


class Restatement:
    """DESIGN.md 30's semantics over Python lists: the reference the streams are checked against.  target and base come from their
    definitions ((N + i) // E and a running sum), not from the closed forms of the core."""

    def __init__(self, E, N):
        self.E, self.N = E, N
        self.target = [(N + i) // E for i in range(E)]
        self.base, s = [], 0
        for i in range(E):
            self.base.append(s)
            s += self.target[i]
        assert s == N
        self.cur_ret, self.cur_len, self.count = [0.0] * E, [0] * E, [0] * E
        self.remaining, self.records = N, [[0.0, 0.0, 0.0] for _ in range(N)]

    def step(self, rew, done, success, keep=None):
        wrote = 0
        for i in range(self.E):
            c = 1 if keep is None else int(keep[i] != 0)
            if c:
                self.cur_ret[i] = self.cur_ret[i] + float(rew[i])
                self.cur_len[i] += 1
            if done[i]:
                if self.count[i] < self.target[i]:
                    self.records[self.base[i] + self.count[i]] = [self.cur_ret[i], float(self.cur_len[i]), 1.0 if success[i] else 0.0]
                    self.count[i] += 1
                    wrote += 1
                self.cur_ret[i], self.cur_len[i] = 0.0, 0
        self.remaining -= wrote
        return wrote

    def written(self):
        """bool [N]: the slots that hold a record"""
        w = [False] * self.N
        for i in range(self.E):
            for k in range(self.count[i]):
                w[self.base[i] + k] = True
        return w

    def lists(self):
        """(episode_rewards, episode_lengths, episode_successes) in slot (env-major) order"""
        return [r[0] for r in self.records], [int(r[1]) for r in self.records], [bool(r[2]) for r in self.records]


def run_to_end(E, N, use_keep, sinks, after_step=None, extra=10, limit=10000):
    """feed one scripted stream to every sink (objects with step(rew, done, success, keep)) until the Restatement among them - sinks[0] -
    has remaining == 0, plus `extra` further steps; after_step(t, wrote) runs after each one.  Returns the number of steps."""
    stream, ref, t, tail = Stream(E, use_keep), sinks[0], 0, 0
    while ref.remaining > 0 or tail < extra:
        tail += 1 if ref.remaining == 0 else 0
        rew, done, succ, keep = stream.next()
        wrote = ref.step(rew, done, succ, keep)
        for s in sinks[1:]:
            s.step(rew, done, succ, keep)
        t += 1
        if after_step:
            after_step(t, wrote)
        assert t < limit
    return t


def summary_fixed_order(records, written):
    """csrc/xarm_eval_core.h's summary restated in NumPy float64 scalars: thread t of 256 sums the written slots t, t + 256, ... in slot
    order from 0.0, the partials are added in thread order starting from thread 0's, twice (means, then squared deviations)."""
    rec = np.asarray(records, np.float64)
    own = [[s for s in range(t, len(rec), THREADS) if written[s]] for t in range(THREADS)]

    def merged(f):
        parts = []
        for slots in own:
            acc = np.float64(0.0)
            for s in slots:
                acc = acc + f(s)
            parts.append(acc)
        tot = parts[0]
        for p in parts[1:]:
            tot = tot + p
        return tot
    n = np.float64(sum(len(slots) for slots in own))
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_r, mean_l = merged(lambda s: rec[s, 0]) / n, merged(lambda s: rec[s, 1]) / n
        sq_r = merged(lambda s: (rec[s, 0] - mean_r) * (rec[s, 0] - mean_r))
        sq_l = merged(lambda s: (rec[s, 1] - mean_l) * (rec[s, 1] - mean_l))
        succ = np.float64(sum(1 for slots in own for s in slots if rec[s, 2] != 0.0)) / n
        vals = [rec[s, 0] for slots in own for s in slots]
        return np.array([mean_r, np.sqrt(sq_r / n), mean_l, np.sqrt(sq_l / n), succ, min(vals) if vals else mean_r, max(vals) if vals else mean_r, n])


# ---- scripted CPU envs for evaluate_policy_torch, the callback and the drivers
class StreamEnv:
    """A goal VecEnv on the host whose rewards, dones and successes are the scripted stream's (lazy=True: with info["resetting"] = the
    stream's masked steps), with what the drivers read.  flat=True presents the observation tensor alone."""

    def __init__(self, E, lazy=False, flat=False, obs_dim=5, goal_dim=3, act_dim=2):
        self.num_envs, self.device, self.lazy, self.flat_observation = E, torch.device("cpu"), lazy, flat
        self.obs_dim, self.goal_dim, self.act_dim, self.action_dim = obs_dim, 0 if flat else goal_dim, act_dim, act_dim
        self._gd = goal_dim
        self.max_episode_steps = max(ep_lens(E))
        self.stream, self.closed, self.actions = Stream(E, lazy), False, []

    def _obs(self):
        e = torch.arange(self.num_envs, dtype=torch.float32)[:, None]
        o = e * 0.125 + torch.arange(self.obs_dim, dtype=torch.float32)[None, :] + 0.5 * self.stream.t
        if self.flat_observation:
            return o
        return {"observation": o, "achieved_goal": o[:, :self._gd].clone(), "desired_goal": torch.ones(self.num_envs, self._gd)}

    def achieved_goal_of(self, obs):
        return obs[..., :self._gd]

    def compute_reward(self, ag, g, info):
        return (torch.linalg.norm(ag - g, dim=-1) < 0.05).to(torch.float32)

    def reset(self):
        self.stream = Stream(self.num_envs, self.lazy)
        return self._obs()

    def step(self, a):
        assert tuple(a.shape) == (self.num_envs, self.act_dim) and float(a.abs().max()) <= 1.0
        self.actions.append(a.clone())
        term = self._obs()
        rew, done, succ, keep = self.stream.next()
        info = {"is_success": torch.from_numpy(succ), "terminal_observation": term if self.flat_observation else term["observation"],
                "TimeLimit.truncated": torch.from_numpy(done != 0) & torch.from_numpy(succ == 0)}
        if keep is not None:
            info["resetting"] = torch.from_numpy(keep == 0)
        return self._obs(), torch.from_numpy(rew), torch.from_numpy(done), info

    def close(self):
        self.closed = True


def expected_lists(E, N, lazy=False):
    """(Restatement after the scripted stream ran until remaining == 0, the steps that took)"""
    ref = Restatement(E, N)
    steps = run_to_end(E, N, lazy, [ref], extra=0)
    return ref, steps
