"""Policy evaluation for the batched envs: stable-baselines3's `evaluate_policy` and `EvalCallback`, and the counterpart of the
reference's `benchmark/display.py` (load the agent, `env.training = False`, `model.predict(obs, deterministic=True)`, report reward and
success per episode).  DESIGN.md 30.

With E = env.num_envs, N = n_eval_episodes and q, r = divmod(N, E), env i contributes its FIRST target[i] = (N + i) // E episodes after
`env.reset()` - SB3's split, which keeps the estimate from favouring short episodes.  Per step cur_ret += c * rew and cur_len += c with
c = 1, or the keep mask of lazy auto-reset (~info["resetting"]), as train.EpisodeMonitor counts; where an env is done and still below its
target, (cur_ret, cur_len, info["is_success"]) is recorded; the accumulators are float64 as SB3's are.  Episode k of env i lands in the
fixed slot base[i] + k (base = the exclusive prefix of target), so the episode lists are SB3's up to order: env-major here, arrival
order there.  Mean and std do not depend on the order.

`DeviceEvaluator` keeps this accounting on the device (csrc/xarm_k_eval.hip: one launch per step, one 4-byte host read per
`check_every` steps); `evaluate_policy_torch` is the same in torch ops with SB3's host read on every step - the checker, and the path of
a CPU env.

  python -m gym_xarm_amd.evaluation --checkpoint runs/reach/best_eval_model.safetensors --env XarmReach-v0 --num-envs 1024 --episodes 1024
"""
import argparse
import ctypes as C
import json
import os

import numpy as np
import torch

RESULT_KEYS = ("mean_reward", "std_reward", "mean_length", "std_length", "success_rate", "min_reward", "max_reward", "n_episodes")


def quotas(num_envs, n_eval_episodes):
    """(target, base): int64 [E] each - the episodes env i contributes and the slot of its first record"""
    E, N = int(num_envs), int(n_eval_episodes)
    q, r = divmod(N, E)
    i = torch.arange(E, dtype=torch.int64)
    return q + (i >= E - r).to(torch.int64), q * i + (i - (E - r)).clamp(min=0)


def _check_n(n_eval_episodes):
    if int(n_eval_episodes) < 1:
        raise ValueError("n_eval_episodes must be >= 1, not %r" % (n_eval_episodes,))
    return int(n_eval_episodes)


def _flat(obs):
    return torch.cat([obs["observation"], obs["achieved_goal"], obs["desired_goal"]], dim=1) if isinstance(obs, dict) else obs


# ------------------------------------------------------------------------------------------------------------- the policy callable
class _Policy:
    """obs -> env_action for one model, with frozen normalisation; `kind` names the path taken ("device" or "torch")"""

    def __init__(self, model, normalize, deterministic):
        from . import device_policy, device_sac, device_td3, sac, td3
        from .train import ActorCritic
        self.normalize, self.deterministic = normalize, bool(deterministic)
        self.device_stats = normalize is not None and hasattr(normalize, "stats")      # a DeviceVecNormalize
        self.runner, self.family = None, None
        if isinstance(model, device_policy.DevicePolicy):
            self.runner, self.model, self.family = model, model.model, "ac"
        elif isinstance(model, device_sac.DeviceSAC):
            self.runner, self.model, self.family = model, model.model, "sac"
        elif isinstance(model, device_td3.DeviceTD3):
            self.runner, self.model, self.family = model, model.model, "td3"
        elif isinstance(model, ActorCritic):
            self.model, self.family = model, "ac"
        elif isinstance(model, sac.SacPolicy):
            self.model, self.family = model, "sac"
        elif isinstance(model, td3.Td3Policy):
            self.model, self.family = model, "td3"
        else:
            raise TypeError("as_policy takes an ActorCritic, a DevicePolicy, a SacPolicy / DeviceSAC, a Td3Policy / DeviceTD3 or a callable, not %s"
                            % type(model).__name__)
        self.device = next(self.model.parameters()).device
        if self.runner is None and self.device.type == "cuda":
            # the shapes the device classes evaluate go through their kernels; they refuse every other shape with a ValueError and the
            # torch expression of the drivers takes it
            try:
                if self.family == "ac":
                    self.runner = device_policy.DevicePolicy(model)
                elif self.family == "sac":
                    self.runner = device_sac.DeviceSAC(model, 1)
                else:
                    self.runner = device_td3.DeviceTD3(model, 1)
            except ValueError:
                self.runner = None
        self.kind = "device" if self.runner is not None and self.device.type == "cuda" else "torch"
        self._out = self._nobs = None
        self.action_noise = float(self.runner.hyper["action_noise"]) if self.family == "td3" and self.runner is not None else 0.1

    def _sized(self, E):
        if self._out is None or self._out["env_action"].shape[0] != E:
            A = int(self.runner.act_dim)
            self._out = {"action": torch.empty(E, A, device=self.device), "env_action": torch.empty(E, A, device=self.device)}
            self._nobs = torch.empty(E, int(self.runner.obs_width), device=self.device)
            if self.family != "ac" and getattr(self.runner, "backend", "wide") == "wide":      # DevicePolicy sizes its own in act_into
                self.runner.reserve_act(E)

    def _normalized(self, obs):
        """the [E, D] input row of the learners' actors: the frozen statistics applied, nothing updated"""
        if self.normalize is None:
            return _flat(obs)
        if self.device_stats and self.kind == "device":
            parts = (obs["observation"], obs["achieved_goal"], obs["desired_goal"]) if isinstance(obs, dict) else (obs,)
            return self.normalize.normalize_rows(self._nobs, *parts)
        from .sac import _frozen_norm
        return _frozen_norm(self.normalize, _flat(obs))

    def __call__(self, obs):
        if self.kind == "device":
            self._sized(int((obs["observation"] if isinstance(obs, dict) else obs).shape[0]))
            if self.family == "ac":
                if self.normalize is None or self.device_stats:
                    return self.runner.act_into(self._out, obs, self.deterministic, self.normalize)["env_action"]
                return self.runner.act_into(self._out, self._normalized(obs).contiguous(), self.deterministic)["env_action"]
            nobs = self._normalized(obs).contiguous()
            if self.family == "sac":
                return self.runner.act_into({"action": self._out["env_action"]}, nobs, self.deterministic)["action"]
            return self.runner.act_into(self._out["env_action"], nobs, "deterministic" if self.deterministic else "gaussian")
        with torch.no_grad():
            x = self._normalized(obs)
            if self.family == "ac":
                d = self.model.dist(x)
                return (d.mean if self.deterministic else d.sample()).clamp(-1, 1)
            if self.family == "sac":
                return self.model.action_log_prob(x, deterministic=self.deterministic)[0]
            a = self.model.action(x)
            return a if self.deterministic else (a + self.action_noise * torch.randn_like(a)).clamp(-1.0, 1.0)


def as_policy(model_or_learner, normalize=None, deterministic=True):
    """The callable obs -> env_action that the evaluators take.

    model_or_learner: a train.ActorCritic or DevicePolicy, a sac.SacPolicy or DeviceSAC, a td3.Td3Policy or DeviceTD3 - or any other
    callable, which is returned as it is.  On a GPU the shapes the device classes support run through their `act_into` with outputs
    allocated once (capturable); every other shape, and a CPU model, takes the torch expression of the drivers:
    `dist(x).mean.clamp(-1, 1)`, `tanh(mean)`, the TD3 actor (deterministic=False: the drivers' exploring action).
    normalize: a DeviceVecNormalize or train.VecNormalize whose statistics are applied FROZEN to the raw observation and never updated -
    SB3's sync_envs_normalization, `training = False` and `norm_reward = False` in one step; the evaluators account raw rewards.  The
    model's parameters and a DeviceVecNormalize's statistics are read in place on every call."""
    from .device_policy import DevicePolicy
    from .device_sac import DeviceSAC
    from .device_td3 import DeviceTD3
    if isinstance(model_or_learner, _Policy):
        return model_or_learner
    from .sac import SacPolicy
    from .td3 import Td3Policy
    from .train import ActorCritic
    if isinstance(model_or_learner, (ActorCritic, SacPolicy, Td3Policy, DevicePolicy, DeviceSAC, DeviceTD3)):
        return _Policy(model_or_learner, normalize, deterministic)
    if callable(model_or_learner):
        return model_or_learner
    raise TypeError("as_policy takes a model, a device learner or a callable, not %s" % type(model_or_learner).__name__)


# ------------------------------------------------------------------------------------------------------------- the device evaluator
class DeviceEvaluator:
    """SB3's evaluate_policy accounting with its state on the device and the step in one HIP launch (csrc/xarm_k_eval.hip).

    State (device tensors): `cur_ret` float64 [E], `cur_len` / `count` int32 [E], `remaining` int32 [1] and `records` float64 [N, 3] =
    (return, length, success) with episode k of env i at slot base[i] + k; `episode_rewards`, `episode_lengths` and `episode_successes`
    are views of the records' columns - SB3's lists up to order (env-major here, whichever env finished first there).
    `step_into(rew, done, success, keep)` is the capturable call: no allocation, no host read."""

    def __init__(self, env, n_eval_episodes):
        from . import _native
        self.env, self.n_eval_episodes = env, _check_n(n_eval_episodes)
        self.num_envs, self.device = int(env.num_envs), torch.device(env.device)
        if self.device.type != "cuda":
            raise ValueError("DeviceEvaluator keeps the episode accounting on the GPU and steps it with a HIP kernel: the env is on '%s'.  "
                             "There is no host path; evaluate_policy_torch is the torch implementation." % self.device)
        self._L, self._check = _native.load(), _native.check
        E, N, dev = self.num_envs, self.n_eval_episodes, self.device
        self.layout = _native.XarmEvalLayout(E, N)
        self.cur_ret = torch.zeros(E, device=dev, dtype=torch.float64)
        self.cur_len = torch.zeros(E, device=dev, dtype=torch.int32)
        self.count = torch.zeros(E, device=dev, dtype=torch.int32)
        self.remaining = torch.full((1,), N, device=dev, dtype=torch.int32)
        self.records = torch.zeros(N, 3, device=dev, dtype=torch.float64)
        self.out = torch.zeros(8, device=dev, dtype=torch.float64)
        self.steps = 0
        self._graph = self._graph_policy = self._graph_obs = None

    episode_rewards = property(lambda self: self.records[:, 0])
    episode_lengths = property(lambda self: self.records[:, 1])
    episode_successes = property(lambda self: self.records[:, 2])

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _state(self):
        return [C.c_void_p(t.data_ptr()) for t in (self.cur_ret, self.cur_len, self.count, self.remaining, self.records)]

    def _u8(self, x, what):
        if x.dtype == torch.bool and x.is_contiguous():
            x = x.view(torch.uint8)                  # same bytes, no copy
        if x.dtype != torch.uint8 or not x.is_contiguous():
            x = (x != 0).to(torch.uint8).contiguous()
        assert x.shape == (self.num_envs,) and x.device == self.records.device, what
        return x

    def begin(self):
        """zero the accumulators and the records, count = 0, remaining = N (one launch)"""
        self._check(self._L, None, self._L.xarm_eval_begin(C.byref(self.layout), *self._state(), self._stream()), "xarm_eval_begin")
        self.steps = 0

    def step_into(self, rew, done, success, keep=None):
        """One env step's accounting: rew float32 [E], done and success uint8 / bool [E] as the VecEnv returns them (read in place),
        keep uint8 / bool [E] or None.  One launch on the current stream; no allocation, no host read; capturable."""
        assert rew.dtype == torch.float32 and rew.is_contiguous() and rew.shape == (self.num_envs,) and rew.device == self.records.device, "rew"
        done, success = self._u8(done, "done"), self._u8(success, "success")
        keep = None if keep is None else self._u8(keep, "keep")
        rc = self._L.xarm_eval_step(C.byref(self.layout), *self._state(), C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr()),
                                    C.c_void_p(success.data_ptr()), None if keep is None else C.c_void_p(keep.data_ptr()), self._stream())
        self._check(self._L, None, rc, "xarm_eval_step")

    def summary(self):
        """`out` float64 [8] on the device: RESULT_KEYS over the records written so far (one launch, fixed summation order)"""
        rc = self._L.xarm_eval_summary(C.byref(self.layout), C.c_void_p(self.count.data_ptr()), C.c_void_p(self.records.data_ptr()),
                                       C.c_void_p(self.out.data_ptr()), self._stream())
        self._check(self._L, None, rc, "xarm_eval_summary")
        return self.out

    def _iterate(self, policy, obs):
        obs, rew, done, info = self.env.step(policy(obs))
        self.step_into(rew, done, info["is_success"], ~info["resetting"] if "resetting" in info else None)
        return obs

    def _capture(self, policy, obs):
        """one eager iteration on a side stream - it is the evaluation's next step - then the capture of one iteration (which runs nothing)"""
        cur, side = torch.cuda.current_stream(self.device), torch.cuda.Stream(self.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            nobs = self._iterate(policy, obs)
        cur.wait_stream(side)
        same = lambda a, b: a.data_ptr() == b.data_ptr()
        if isinstance(obs, dict) != isinstance(nobs, dict) or not (all(same(obs[k], nobs[k]) for k in obs) if isinstance(obs, dict) else same(obs, nobs)):
            raise ValueError("graph=True replays one captured iteration: it needs an env that rewrites its observation tensors in place")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._iterate(policy, nobs)
        self._graph, self._graph_policy, self._graph_obs = graph, policy, nobs
        return nobs

    def run(self, policy, check_every=None, graph=False):
        """Evaluate `policy` (as_policy's callable: obs -> env_action) for n_eval_episodes episodes: env.reset(), begin(), then
        policy -> env.step -> step_into until `remaining` is 0, which the host reads (4 bytes) every `check_every` steps only - default
        env.max_episode_steps, about once per quota round.  Returns a dict of floats: RESULT_KEYS and `steps`, the env steps taken.
        graph=True: one iteration is captured in a torch.cuda.graph after one eager iteration on a side stream (that iteration is the
        run's first step) and replayed between the reads.  The policy's parameters and the normaliser's statistics are read in place, so
        the capture serves every later run of this evaluator with the same policy object; another policy is captured anew."""
        check_every = max(1, int(getattr(self.env, "max_episode_steps", 50) if check_every is None else check_every))
        if graph and not getattr(policy, "kind", "device") == "device":
            raise ValueError("graph=True captures the device path: this policy takes the torch expression (a CPU model, an unsupported shape)")
        if graph and getattr(policy, "normalize", None) is not None and not getattr(policy, "device_stats", True):
            raise ValueError("graph=True reads the normaliser's statistics in place: it takes a DeviceVecNormalize (train.VecNormalize rebinds its tensors)")
        obs = self.env.reset()
        self.begin()
        while True:
            k = 0
            if graph and (self._graph is None or self._graph_policy is not policy):
                obs = self._capture(policy, obs)
                k = 1
            for _ in range(k, check_every):
                if graph:
                    self._graph.replay()
                else:
                    obs = self._iterate(policy, obs)
            self.steps += check_every
            if int(self.remaining.item()) <= 0:
                break
        res = dict(zip(RESULT_KEYS, self.summary().tolist()))
        res["n_episodes"] = int(res["n_episodes"])
        res["steps"] = self.steps
        return res


# ------------------------------------------------------------------------------------------------------------- the torch evaluator
class TorchAccounting:
    """the accounting of the module docstring in torch ops, on the device of the tensors it is fed: `step` is one env step and returns
    SB3's loop condition `(count < target).any()` - a host read.  `records` float64 [N, 3] in slot order."""

    def __init__(self, num_envs, n_eval_episodes, device):
        self.E, self.N = int(num_envs), _check_n(n_eval_episodes)
        self.target, self.base = (x.to(device) for x in quotas(self.E, self.N))
        self.count = torch.zeros(self.E, dtype=torch.int64, device=device)
        self.cur_ret = torch.zeros(self.E, dtype=torch.float64, device=device)
        self.cur_len = torch.zeros(self.E, dtype=torch.int64, device=device)
        self._rec = torch.zeros(self.N + 1, 3, dtype=torch.float64, device=device)       # row N is a dump slot

    records = property(lambda self: self._rec[:self.N])

    def step(self, rew, done, success, keep=None):
        fin = done != 0
        if keep is not None:
            self.cur_ret = self.cur_ret + torch.where(keep, rew.to(torch.float64), torch.zeros_like(self.cur_ret))
            self.cur_len = self.cur_len + keep.to(torch.int64)
        else:
            self.cur_ret = self.cur_ret + rew.to(torch.float64)
            self.cur_len = self.cur_len + 1
        write = fin & (self.count < self.target)
        pos = torch.where(write, self.base + self.count, torch.full_like(self.count, self.N))
        self._rec[pos] = torch.stack([self.cur_ret, self.cur_len.to(torch.float64), (success != 0).to(torch.float64)], dim=1)
        self.count = self.count + write.to(torch.int64)
        self.cur_ret = torch.where(fin, torch.zeros_like(self.cur_ret), self.cur_ret)
        self.cur_len = torch.where(fin, torch.zeros_like(self.cur_len), self.cur_len)
        return bool((self.count < self.target).any())


def evaluate_policy_torch(model, env, n_eval_episodes=10, deterministic=True, normalize=None, return_episode_rewards=False,
                          reward_threshold=None, full=False):
    """evaluate_policy in torch ops on any VecEnv (a CPU env included): the semantics of the module docstring with SB3's loop
    `while (count < target).any()` - one host read per step (TorchAccounting).  full=True returns (result dict as DeviceEvaluator.run's,
    records float64 [N, 3] in slot order) instead."""
    N, E = _check_n(n_eval_episodes), int(env.num_envs)
    policy = as_policy(model, normalize, deterministic)
    acc = TorchAccounting(E, N, torch.device(env.device))
    obs, steps, more = env.reset(), 0, True
    while more:
        obs, rew, done, info = env.step(policy(obs))
        steps += 1
        more = acc.step(rew, done, info["is_success"], ~info["resetting"] if "resetting" in info else None)
    records = acc.records
    r, l = records[:, 0].cpu().numpy(), records[:, 1].cpu().numpy()
    mean_reward, std_reward = float(np.mean(r)), float(np.std(r))
    if reward_threshold is not None:
        assert mean_reward > reward_threshold, "Mean reward below threshold: %.2f < %.2f" % (mean_reward, reward_threshold)
    if full:
        res = {"mean_reward": mean_reward, "std_reward": std_reward, "mean_length": float(np.mean(l)), "std_length": float(np.std(l)),
               "success_rate": float(records[:, 2].mean()), "min_reward": float(r.min()), "max_reward": float(r.max()), "n_episodes": N,
               "steps": steps}
        return res, records
    if return_episode_rewards:
        return r.tolist(), [int(x) for x in l]
    return mean_reward, std_reward


def evaluate_policy(model, env, n_eval_episodes=10, deterministic=True, normalize=None, return_episode_rewards=False, reward_threshold=None,
                    backend=None, graph=False):
    """SB3's evaluate_policy for a batched env: (mean_reward, std_reward) - np.std's population std - of n_eval_episodes episodes split over
    the envs as the module docstring says, or with return_episode_rewards the lists (episode_rewards, episode_lengths), which are SB3's up
    to order (env-major).  model: anything as_policy takes; normalize: the VecNormalize / DeviceVecNormalize whose frozen statistics
    normalise the observation.  reward_threshold: asserts mean_reward above it, as SB3.  backend: "device" (DeviceEvaluator; the default
    on a GPU env) or "torch" (evaluate_policy_torch; the default elsewhere).  graph: DeviceEvaluator.run's."""
    backend = ("device" if torch.device(env.device).type == "cuda" else "torch") if backend is None else backend
    if backend not in ("device", "torch"):
        raise ValueError("backend must be None, 'device' or 'torch', not %r" % (backend,))
    if backend == "torch":
        return evaluate_policy_torch(model, env, n_eval_episodes, deterministic, normalize, return_episode_rewards, reward_threshold)
    ev = DeviceEvaluator(env, n_eval_episodes)
    res = ev.run(as_policy(model, normalize, deterministic), graph=graph)
    if reward_threshold is not None:
        assert res["mean_reward"] > reward_threshold, "Mean reward below threshold: %.2f < %.2f" % (res["mean_reward"], reward_threshold)
    if return_episode_rewards:
        return ev.episode_rewards.tolist(), [int(x) for x in ev.episode_lengths.tolist()]
    return res["mean_reward"], res["std_reward"]


# ------------------------------------------------------------------------------------------------------------- the callback
class EvalCallback:
    """SB3's EvalCallback beside train.SaveOnBestTrainingRewardCallback: every `eval_freq` calls of `on_step(model, venv, num_timesteps)`
    the model is evaluated on `eval_env` for n_eval_episodes episodes with venv's statistics frozen (they, the model and the training
    env are left as they are).  Keeps `evaluations_timesteps`, `evaluations_results` [n, N], `evaluations_length`, `evaluations_successes`,
    `last_mean_reward`, `best_mean_reward`, `last_success_rate`; with log_dir rewrites `<log_dir>/evaluations.npz` (SB3's keys timesteps,
    results, ep_lengths, successes) and saves `<log_dir>/best_eval_model.safetensors` (train.save_model) when the mean improved.  On a GPU
    env the evaluator is a DeviceEvaluator built once; graph=True replays its captured iteration on every evaluation."""

    def __init__(self, eval_env, n_eval_episodes=None, eval_freq=10000, log_dir=None, deterministic=True, graph=False, verbose=1):
        self.eval_env = eval_env
        self.n_eval_episodes = _check_n(int(eval_env.num_envs) if n_eval_episodes is None else n_eval_episodes)
        self.eval_freq, self.log_dir, self.deterministic, self.graph, self.verbose = int(eval_freq), log_dir, deterministic, bool(graph), verbose
        if self.eval_freq < 1:
            raise ValueError("eval_freq must be >= 1")
        self.device_backend = torch.device(eval_env.device).type == "cuda"
        self.evaluator = DeviceEvaluator(eval_env, self.n_eval_episodes) if self.device_backend else None
        self._policy = self._policy_key = None
        self.n_calls, self.saves = 0, 0
        self.evaluations_timesteps, self.evaluations_results, self.evaluations_length, self.evaluations_successes = [], [], [], []
        self.last_mean_reward, self.best_mean_reward, self.last_success_rate = -float("inf"), -float("inf"), float("nan")
        self.save_path = self.npz_path = None
        if log_dir is not None:
            os.makedirs(log_dir, exist_ok=True)
            self.save_path, self.npz_path = os.path.join(log_dir, "best_eval_model.safetensors"), os.path.join(log_dir, "evaluations.npz")

    def evaluate(self, model, venv):
        """one evaluation now: (result dict, records float64 [N, 3] on the host)"""
        if self._policy is None or self._policy_key != (id(model), id(venv)):
            self._policy, self._policy_key = as_policy(model, venv, self.deterministic), (id(model), id(venv))
        if self.device_backend:
            res = self.evaluator.run(self._policy, graph=self.graph)
            return res, self.evaluator.records.cpu()
        res, rec = evaluate_policy_torch(self._policy, self.eval_env, self.n_eval_episodes, full=True)
        return res, rec.cpu()

    def on_step(self, model, venv, num_timesteps):
        self.n_calls += 1
        if self.n_calls % self.eval_freq:
            return True
        res, rec = self.evaluate(model, venv)
        self.evaluations_timesteps.append(int(num_timesteps))
        self.evaluations_results.append(rec[:, 0].tolist())
        self.evaluations_length.append([int(x) for x in rec[:, 1].tolist()])
        self.evaluations_successes.append([bool(x) for x in rec[:, 2].tolist()])
        self.last_mean_reward, self.last_success_rate, self.last_result = res["mean_reward"], res["success_rate"], res
        if self.npz_path is not None:
            np.savez(self.npz_path, timesteps=np.asarray(self.evaluations_timesteps), results=np.asarray(self.evaluations_results),
                     ep_lengths=np.asarray(self.evaluations_length), successes=np.asarray(self.evaluations_successes))
        if self.verbose > 0:
            print("Eval num_timesteps={}, episode_reward={:.2f} +/- {:.2f}, success rate {:.2%}".format(
                num_timesteps, res["mean_reward"], res["std_reward"], res["success_rate"]))
        if res["mean_reward"] > self.best_mean_reward:
            self.best_mean_reward = res["mean_reward"]
            if self.save_path is not None:
                from .train import save_model
                if self.verbose > 0:
                    print("New best mean reward: saving {}".format(self.save_path))
                save_model(self.save_path, model, venv)
                self.saves += 1
        return True


def make_eval_callback(eval_freq, n_eval_episodes, eval_envs, eval_env, eval_graph, env_id, num_envs, seed, config, log_dir, quiet):
    """the drivers' EvalCallback (train, sac.train_off_policy): None when eval_freq is None; else on `eval_env`, or on a second env
    make(env_id, num_envs=eval_envs or min(num_envs, 1024), seed=seed + 1, config=config, auto_reset=True), with n_eval_episodes
    defaulting to one per eval env"""
    if eval_freq is None:
        return None
    if eval_env is None:
        import gym_xarm_amd
        eval_env = gym_xarm_amd.make(env_id, num_envs=int(eval_envs or min(num_envs, 1024)), seed=seed + 1, config=config, auto_reset=True)
    return EvalCallback(eval_env, n_eval_episodes, eval_freq, log_dir, graph=eval_graph, verbose=0 if quiet else 1)


# ------------------------------------------------------------------------------------------------------------- the CLI
def checkpoint_algo(path):
    """the learner family of a checkpoint written by train.save_model: the metadata's `algo` where present, else read off the tensors'
    names ("a2c" stands for both on-policy learners: they share the ActorCritic)"""
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        meta, keys = f.metadata() or {}, set(f.keys())
    if "algo" in meta:
        return meta["algo"]
    if "policy.log_alpha" in keys:
        return "sac"
    if any(k.startswith("policy.actor_target.") for k in keys):
        return "td3"
    return "a2c"


def load_agent(path, env, algo=None, device=None):
    """(model on the env's device, normaliser or None) of a checkpoint: train / sac / td3.load_checkpoint by `algo` (None:
    checkpoint_algo) and the normaliser rebuilt from the file's `vecnormalize.*` entries - a DeviceVecNormalize on a GPU env"""
    from . import sac, td3, train
    algo = checkpoint_algo(path) if algo is None else algo
    load = {"a2c": train.load_checkpoint, "ppo": train.load_checkpoint, "sac": sac.load_checkpoint, "td3": td3.load_checkpoint}[algo]
    model, vn = load(path)
    dev = torch.device(env.device if device is None else device)
    model = model.to(dev)
    normalize = None
    if vn:
        if dev.type == "cuda":
            from .normalize import DeviceVecNormalize
            normalize = DeviceVecNormalize(env)
        else:
            normalize = train.VecNormalize(env)
        normalize.load_state_dict(vn)
        normalize.training = False
    return model, normalize


def main(argv=None, env=None):
    """env: an already built VecEnv (tests); None: gym_xarm_amd.make(--env, --num-envs, seed --seed)"""
    ap = argparse.ArgumentParser(description="evaluate a checkpoint: deterministic reward and success rate over N episodes")
    ap.add_argument("--checkpoint", required=True, help="a file written by train.save_model (--save, best_model / best_eval_model.safetensors)")
    ap.add_argument("--env", default="XarmReach-v0")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=None, help="n_eval_episodes (default: one per env)")
    ap.add_argument("--algo", choices=("a2c", "ppo", "sac", "td3"), default=None, help="default: the checkpoint's metadata, else its tensor names")
    ap.add_argument("--reward-type", default="dense")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--stochastic", action="store_true", help="sample the action instead of taking the deterministic one")
    ap.add_argument("--graph", action="store_true", help="replay one captured iteration (DeviceEvaluator.run graph=True)")
    ap.add_argument("--frames-dir", default=None, help="save env.render of the first --frame-envs envs after every step as .npy")
    ap.add_argument("--frame-envs", type=int, default=1)
    args = ap.parse_args(argv)
    env = make_cli_env(args) if env is None else env
    try:
        model, normalize = load_agent(args.checkpoint, env, args.algo)
        policy = as_policy(model, normalize, deterministic=not args.stochastic)
        N = int(env.num_envs) if args.episodes is None else args.episodes
        if args.frames_dir:
            os.makedirs(args.frames_dir, exist_ok=True)
            inner, frame = policy, [0]

            def policy(obs):
                if frame[0] > 0:       # the observation after a step: the scene it shows
                    rgb = env.render(mode="rgb_array", env_ids=list(range(min(args.frame_envs, int(env.num_envs)))))
                    np.save(os.path.join(args.frames_dir, "frame_%06d.npy" % frame[0]), np.asarray(rgb.cpu() if torch.is_tensor(rgb) else rgb))
                frame[0] += 1
                return inner(obs)
        if torch.device(env.device).type == "cuda":
            res = DeviceEvaluator(env, N).run(policy, graph=args.graph and not args.frames_dir)
        else:
            res, _ = evaluate_policy_torch(policy, env, N, full=True)
        res.update(env=args.env, num_envs=int(env.num_envs), algo=args.algo or checkpoint_algo(args.checkpoint), deterministic=not args.stochastic)
        print(json.dumps(res), flush=True)
        return res
    finally:
        env.close()


def make_cli_env(args):
    import gym_xarm_amd
    cfg = {"reward_type": args.reward_type, "GUI": False} if ("Reach" in args.env or "PickAndPlace" in args.env) else None
    if "Handover" in args.env and "NoGoal" not in args.env:
        cfg = {"reward_type": args.reward_type}
    return gym_xarm_amd.make(args.env, num_envs=args.num_envs, seed=args.seed, config=cfg, auto_reset=True)


if __name__ == "__main__":
    main()
