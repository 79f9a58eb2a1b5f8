"""On-device A2C training driver for the batched envs - the MI355X counterpart of the reference's
`benchmark/train.py:65-111` (SB3: make_vec_env -> VecNormalize(norm_obs, norm_reward, clip_obs=10) -> A2C
'MlpPolicy' -> learn -> save).  Everything (env step, normalisation statistics, policy, optimiser) stays on the
GPU; there is no host round trip per step.  SB3 itself is not installed here, so the A2C update (n_steps = 5,
gamma 0.99, GAE lambda 1, value coefficient 0.5, entropy coefficient 0, RMSprop 7e-4 - SB3's defaults) is written
out in ~60 lines of torch.

  python -m gym_xarm_amd.train --env XarmReach-v0 --num-envs 4096 --updates 300 --reward-type dense
"""
import argparse
import json
import math
import os
import time

import torch
import torch.nn as nn


class RunningMeanStd:
    """VecNormalize's running statistics (parallel-variance update), as tensors on the env's device"""

    def __init__(self, shape, device):
        self.mean = torch.zeros(shape, device=device)
        self.var = torch.ones(shape, device=device)
        self.count = 1e-4

    def update(self, x):
        b_mean, b_var, b_n = x.mean(0), x.var(0, unbiased=False), x.shape[0]
        delta, tot = b_mean - self.mean, self.count + b_n
        self.mean = self.mean + delta * b_n / tot
        self.var = (self.var * self.count + b_var * b_n + delta ** 2 * self.count * b_n / tot) / tot
        self.count = tot


class VecNormalize:
    """obs / reward normalisation wrapper (benchmark/train.py:75: norm_obs=True, norm_reward=True, clip_obs=10)"""

    def __init__(self, env, clip_obs=10.0, clip_reward=10.0, gamma=0.99, eps=1e-8):
        self.env, self.clip_obs, self.clip_reward, self.gamma, self.eps = env, clip_obs, clip_reward, gamma, eps
        dev = env.device
        # a flat-observation ('NoGoal') env hands out the observation tensor itself (gym_xarm_amd/sb3_adapter.py FlatObsVecEnv)
        self.flat = bool(getattr(env, "flat_observation", False))
        self.dim = env.obs_dim if self.flat else env.obs_dim + 2 * env.goal_dim
        self.obs_rms = RunningMeanStd((self.dim,), dev)
        self.ret_rms = RunningMeanStd((), dev)
        self.ret = torch.zeros(env.num_envs, device=dev)
        self.training = True

    def _flat(self, obs):
        if self.flat:
            return obs
        return torch.cat([obs["observation"], obs["achieved_goal"], obs["desired_goal"]], dim=1)

    def _norm(self, x, keep=None):
        """keep: bool [E] rows that feed the running statistics (None = all)"""
        if self.training:
            rows = x if keep is None else x[keep]
            if rows.shape[0] > 0:
                self.obs_rms.update(rows)
        return ((x - self.obs_rms.mean) / torch.sqrt(self.obs_rms.var + self.eps)).clamp(-self.clip_obs, self.clip_obs)

    def reset(self):
        self.ret.zero_()
        return self._norm(self._flat(self.env.reset()))

    def step(self, actions):
        obs, rew, done, info = self.env.step(actions)
        # lazy auto-reset: rows that are spending this call on a reset tick (info['resetting']) are not transitions of
        # the task - their observation (desired_goal holds scratch values then) and reward stay out of the statistics
        keep = ~info["resetting"] if "resetting" in info else None
        self.ret = self.ret * self.gamma + rew
        if self.training:
            r = self.ret if keep is None else self.ret[keep]
            if r.shape[0] > 0:
                self.ret_rms.update(r)
        nrew = (rew / torch.sqrt(self.ret_rms.var + self.eps)).clamp(-self.clip_reward, self.clip_reward)
        self.ret = torch.where(done != 0, torch.zeros_like(self.ret), self.ret)
        return self._norm(self._flat(obs), keep), nrew, done, info, rew

    def state_dict(self):
        return {"obs_mean": self.obs_rms.mean, "obs_var": self.obs_rms.var, "obs_count": torch.tensor(float(self.obs_rms.count), dtype=torch.float64),
                "ret_mean": self.ret_rms.mean, "ret_var": self.ret_rms.var, "ret_count": torch.tensor(float(self.ret_rms.count), dtype=torch.float64),
                "clip_obs": torch.tensor(float(self.clip_obs)), "clip_reward": torch.tensor(float(self.clip_reward)),
                "gamma": torch.tensor(float(self.gamma))}

    def load_state_dict(self, sd):
        dev = self.obs_rms.mean.device
        if tuple(sd["obs_mean"].shape) != tuple(self.obs_rms.mean.shape):
            raise ValueError("VecNormalize statistics are for observation width %d, this env has %d" % (sd["obs_mean"].shape[0], self.dim))
        self.obs_rms.mean, self.obs_rms.var = sd["obs_mean"].to(dev).clone(), sd["obs_var"].to(dev).clone()
        self.obs_rms.count = float(sd["obs_count"])
        # files written before the return statistics / clip settings were saved (round 1's --save) hold the observation
        # statistics only: keep this wrapper's own values for what the file lacks
        if "ret_mean" in sd:
            self.ret_rms.mean, self.ret_rms.var = sd["ret_mean"].to(dev).clone(), sd["ret_var"].to(dev).clone()
            self.ret_rms.count = float(sd["ret_count"])
        self.clip_obs = float(sd["clip_obs"]) if "clip_obs" in sd else self.clip_obs
        self.clip_reward = float(sd["clip_reward"]) if "clip_reward" in sd else self.clip_reward
        self.gamma = float(sd["gamma"]) if "gamma" in sd else self.gamma

    def save(self, path):
        """counterpart of `env.save(stats_path)` (benchmark/train.py:107-108): the running statistics and the clip /
        discount settings in one safetensors file (the reference pickles the wrapper; nothing is executed on load here)"""
        from safetensors.torch import save_file
        save_file({k: v.detach().cpu().contiguous() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, env):
        """counterpart of `VecNormalize.load(stats_path, env)` (benchmark/display.py:22)"""
        from safetensors.torch import load_file
        v = cls(env)
        v.load_state_dict(load_file(path))
        return v


class EpisodeMonitor:
    """SB3 `Monitor` for a device-resident batch (benchmark/train.py:74 `monitor_dir`): per-env return and length of
    the running episode are accumulated on the device; every finished episode appends one `r,l,t` row (raw reward sum,
    length, seconds since start) to a device ring, flushed to `<log_dir>/0.monitor.csv` in Monitor's format."""

    def __init__(self, num_envs, device, log_dir=None, env_id="", capacity=1 << 20):
        self.dev, self.log_dir, self.env_id, self.cap = device, log_dir, env_id, capacity
        self.ep_ret = torch.zeros(num_envs, device=device)
        self.ep_len = torch.zeros(num_envs, device=device)
        self.ring = torch.zeros(capacity + 1, 3, device=device)      # r, l, t; row `capacity` is a dump slot
        self.n_dev = torch.zeros((), dtype=torch.long, device=device)   # episodes recorded so far (device counter)
        self.flushed = 0
        self.t_start = time.time()
        self._file = None
        if log_dir is not None:
            os.makedirs(log_dir, exist_ok=True)
            self._file = os.path.join(log_dir, "0.monitor.csv")
            with open(self._file, "w") as f:
                f.write("#%s\n" % json.dumps({"t_start": self.t_start, "env_id": env_id}))
                f.write("r,l,t\n")

    @property
    def n(self):
        return int(self.n_dev.item())

    def update(self, raw_reward, done, count=None):
        """count: bool [E] rows that are real transitions (lazy auto-reset: ~resetting).  No host synchronisation:
        finished envs scatter their row to ring[n + rank among this call's finished envs], the others to the dump slot."""
        c = torch.ones_like(raw_reward) if count is None else count.float()
        self.ep_ret += raw_reward * c
        self.ep_len += c
        fin = done != 0
        rank = torch.cumsum(fin.long(), 0) - 1
        pos = torch.where(fin, (self.n_dev + rank) % self.cap, torch.full_like(rank, self.cap))
        t = torch.full_like(self.ep_ret, time.time() - self.t_start)
        self.ring[pos] = torch.stack([self.ep_ret, self.ep_len, t], dim=1)
        self.n_dev += fin.sum()
        self.ep_ret = torch.where(fin, torch.zeros_like(self.ep_ret), self.ep_ret)
        self.ep_len = torch.where(fin, torch.zeros_like(self.ep_len), self.ep_len)

    def last(self, window=100):
        """(r, l) of the last `window` finished episodes, oldest first"""
        n = self.n
        k = min(window, n, self.cap)
        idx = (torch.arange(n - k, n, device=self.dev)) % self.cap
        return self.ring[idx, 0], self.ring[idx, 1]

    def mean_reward(self, window=100):
        r, _ = self.last(window)
        return float(r.mean()) if r.numel() else None

    def flush(self):
        """append the episodes recorded since the last flush to the CSV"""
        n = self.n
        if self._file is None or n == self.flushed:
            return
        lo = max(self.flushed, n - self.cap)
        idx = (torch.arange(lo, n, device=self.dev)) % self.cap
        rows = self.ring[idx].cpu().tolist()
        with open(self._file, "a") as f:
            for r, l, t in rows:
                f.write("%.6f,%d,%.6f\n" % (r, int(l), t))
        self.flushed = n


class SaveOnBestTrainingRewardCallback:
    """benchmark/train.py:16-47: every `check_freq` calls of env.step, the mean return of the last 100 finished episodes
    is compared with the best so far and the model is saved to `<log_dir>/best_model.safetensors` when it improved
    (policy weights + the VecNormalize statistics that belong to them)."""

    def __init__(self, check_freq, log_dir, monitor, verbose=1):
        self.check_freq, self.log_dir, self.monitor, self.verbose = int(check_freq), log_dir, monitor, verbose
        self.save_path = os.path.join(log_dir, "best_model.safetensors")
        self.best_mean_reward = -float("inf")
        self.n_calls = 0
        self.saves = 0
        os.makedirs(log_dir, exist_ok=True)

    def on_step(self, model, venv, num_timesteps):
        self.n_calls += 1
        if self.n_calls % self.check_freq:
            return True
        self.monitor.flush()
        # the reference's Monitor sees sequential episodes of 4 envs and averages the last 100 (benchmark/train.py:30-33);
        # with thousands of envs finishing in the same call the last 100 entries are one corner of one batch, so the window
        # is widened to at least one episode per env
        mean_reward = self.monitor.mean_reward(max(100, int(self.monitor.ep_ret.numel())))
        if mean_reward is None:
            return True
        if self.verbose > 0:
            print("Num timesteps: {}".format(num_timesteps))
            print("Best mean reward: {:.2f} - Last mean reward per episode: {:.2f}".format(self.best_mean_reward, mean_reward))
        if mean_reward > self.best_mean_reward:
            self.best_mean_reward = mean_reward
            if self.verbose > 0:
                print("Saving new best model to {}".format(self.save_path))
            save_model(self.save_path, model, venv)
            self.saves += 1
        return True


def save_model(path, model, venv):
    from safetensors.torch import save_file
    sd = {"policy." + k: v.detach().cpu().contiguous() for k, v in model.state_dict().items()}
    sd.update({"vecnormalize." + k: v.detach().cpu().contiguous() for k, v in venv.state_dict().items()})
    # a module that records its shape (ActorCritic, sac.SacPolicy) has it written beside the tensors, in the file's metadata: the tensors' keys are
    # the state_dict's for every shape, and load_checkpoint / sac.load_checkpoint rebuild the module from the two entries
    meta = None
    if hasattr(model, "net_arch") and hasattr(model, "activation"):
        meta = {"net_arch": ",".join(str(int(n)) for n in model.net_arch), "activation": str(model.activation)}
        if getattr(model, "algo", None) is not None:        # td3.Td3Policy: td3.load_checkpoint checks it
            meta["algo"] = str(model.algo)
    save_file(sd, path, metadata=meta)


def load_model(path, model, venv):
    from safetensors.torch import load_file
    sd = load_file(path)
    model.load_state_dict({k[len("policy."):]: v for k, v in sd.items() if k.startswith("policy.")})
    venv.load_state_dict({k[len("vecnormalize."):]: v for k, v in sd.items() if k.startswith("vecnormalize.")})


def load_checkpoint(path):
    """(ActorCritic, vecnormalize state) of a checkpoint written by save_model: the module is rebuilt from the metadata entries `net_arch`
    ("256,256,256") and `activation` (a file without them is the 64-64 tanh shape) before its state_dict is loaded; obs_dim and act_dim
    are read off the first and the last layer of `pi`.  sac.load_checkpoint is the same for a SacPolicy."""
    from safetensors import safe_open
    from safetensors.torch import load_file
    with safe_open(path, framework="pt") as f:
        meta = f.metadata() or {}
    sd = load_file(path)
    pol = {k[len("policy."):]: v for k, v in sd.items() if k.startswith("policy.")}
    arch = tuple(int(n) for n in meta["net_arch"].split(",")) if "net_arch" in meta else (64, 64)
    model = ActorCritic(pol["pi.0.weight"].shape[1], pol["pi.%d.bias" % (2 * len(arch))].shape[0], arch, meta.get("activation", "tanh"))
    model.load_state_dict(pol)
    return model, {k[len("vecnormalize."):]: v for k, v in sd.items() if k.startswith("vecnormalize.")}


ACTIVATIONS = {"tanh": nn.Tanh, "relu": nn.ReLU}


class ActorCritic(nn.Module):
    """SB3 'MlpPolicy': separate towers for policy and value, `pi` and `vf`, of len(net_arch) hidden layers each (default: 64-64 tanh),
    and a state-independent log-std.  net_arch: the hidden widths; activation: "tanh" or "relu".  Both are kept as attributes and
    written into a checkpoint's metadata (save_model, load_checkpoint)."""

    def __init__(self, obs_dim, act_dim, net_arch=(64, 64), activation="tanh"):
        super().__init__()
        self.net_arch, self.activation = tuple(int(n) for n in net_arch), str(activation)
        if not self.net_arch or min(self.net_arch) < 1:
            raise ValueError("net_arch must name at least one hidden layer of at least one unit")
        if self.activation not in ACTIVATIONS:
            raise ValueError("activation must be 'tanh' or 'relu', not %r" % (activation,))
        def tower(out):
            layers, last = [], obs_dim
            for width in self.net_arch:
                layers += [nn.Linear(last, width), ACTIVATIONS[self.activation]()]
                last = width
            return nn.Sequential(*layers, nn.Linear(last, out))
        self.pi, self.vf = tower(act_dim), tower(1)
        self.log_std = nn.Parameter(torch.zeros(act_dim))

    def dist(self, x):
        return torch.distributions.Normal(self.pi(x), self.log_std.exp())

    def value(self, x):
        return self.vf(x).squeeze(-1)


# ---- the rollout every learner keeps (TorchA2C, TorchPPO, device_a2c.DeviceA2C, device_ppo.DevicePPO)
def rollout_buffers(T, E, D, A, dev, workspace_bytes=None):
    """obs [T, E, D], action [T, E, A], reward / done / use [T, E]; workspace_bytes: a device update's call workspace as well"""
    b = {"obs": torch.zeros(T, E, D, device=dev), "action": torch.zeros(T, E, A, device=dev), "reward": torch.zeros(T, E, device=dev),
         "done": torch.zeros(T, E, device=dev), "use": torch.ones(T, E, device=dev)}
    if workspace_bytes is not None:
        b["workspace"] = torch.zeros(max(int(workspace_bytes), 16) // 4, dtype=torch.float32, device=dev)
    return b


def store_rollout(b, k, obs, action, reward, done, resetting=None):
    """slot k of the rollout buffers `b`.  A row that spends the call on a lazy-reset tick (`resetting`) carries no reward and no
    gradient and cuts the return like an episode end: reward (1 - resetting), max(done, resetting), use = 1 - resetting.
    action None: the action is already in b["action"][k]."""
    b["obs"][k].copy_(obs)
    if action is not None:
        b["action"][k].copy_(action)
    if resetting is None:
        b["reward"][k].copy_(reward)
        b["done"][k].copy_(done)
        b["use"][k].fill_(1.0)
    else:
        r = resetting.float()
        b["reward"][k].copy_(reward * (1.0 - r))
        b["done"][k].copy_(torch.maximum(done.float(), r))
        b["use"][k].copy_(1.0 - r)


# ---- the torch updates: what train() runs without device_update and what the HIP learners are checked against.  Plain functions of
# a rollout dict (the tensors above, in the model's dtype) and last_obs [E, D], the observation after the rollout's last step.
def _entropy_term(model, loss, ent_coef):
    """(loss - ent_coef entropy, entropy) of the state-independent Gaussian; at ent_coef 0 the term stays out of the graph"""
    entropy = (model.log_std + 0.5 + 0.5 * math.log(2.0 * math.pi)).sum()
    return (loss - ent_coef * entropy if ent_coef != 0.0 else loss), entropy


def a2c_loss(model, rollout, last_obs, gamma=0.99, vf_coef=0.5, ent_coef=0.0):
    """(loss, returns [T, E], terms): n-step returns from the bootstrap value, then policy_loss + vf_coef value_loss - ent_coef entropy
    over the used rows.  terms: policy_loss, value_loss, entropy, n_use and the rows' adv, logp, use, as tensors."""
    O, A, U, rew, done = (rollout[k] for k in ("obs", "action", "use", "reward", "done"))
    with torch.no_grad():
        ret = model.value(last_obs)
        rets = []
        for k in reversed(range(O.shape[0])):
            ret = rew[k] + gamma * ret * (1.0 - done[k])
            rets.append(ret)
        rets = torch.stack(rets[::-1])
    values = model.value(O)
    adv = rets - values.detach()
    logp = model.dist(O).log_prob(A).sum(-1)
    n_use = U.sum().clamp(min=1.0)
    policy_loss, value_sum = -(adv * logp * U).sum() / n_use, (((rets - values) ** 2) * U).sum()
    loss, entropy = _entropy_term(model, policy_loss + vf_coef * value_sum / n_use, ent_coef)
    return loss, rets, {"policy_loss": policy_loss, "value_loss": value_sum / n_use, "entropy": entropy, "n_use": n_use, "adv": adv, "logp": logp, "use": U}


def optimizer_step(model, opt, loss, max_grad_norm=0.5):
    opt.zero_grad(set_to_none=True)
    loss.backward()
    nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)
    opt.step()


def a2c_update(model, opt, rollout, last_obs, gamma=0.99, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5):
    optimizer_step(model, opt, a2c_loss(model, rollout, last_obs, gamma, vf_coef, ent_coef)[0], max_grad_norm)


def ppo_prepare(model, rollout, last_obs, gamma=0.99, gae_lambda=0.95, old_logp=None):
    """flat [N] (adv, ret, old_logp, use) under the model as it is: GAE(gae_lambda) from the rollout's values, ret = adv + value.
    old_logp [T, E]: used in place of the stored actions' log-probabilities."""
    O, A, rew, done = (rollout[k] for k in ("obs", "action", "reward", "done"))
    with torch.no_grad():
        values = model.value(O)
        if old_logp is None:
            old_logp = model.dist(O.flatten(0, 1)).log_prob(A.flatten(0, 1)).sum(-1)
        next_value, next_adv, advs = model.value(last_obs), torch.zeros_like(rew[0]), []
        for k in reversed(range(O.shape[0])):
            keep = 1.0 - done[k]
            delta = rew[k] + gamma * keep * next_value - values[k]
            next_adv = delta + gamma * gae_lambda * keep * next_adv
            next_value = values[k]
            advs.append(next_adv)
        adv = torch.stack(advs[::-1])
    return adv.flatten(), (adv + values).flatten(), old_logp.flatten(), rollout["use"].flatten()


def ppo_old_values(model, rollout):
    """flat [N] values of the rollout's rows under the model as it is - what ppo_prepare's returns were built from, and what
    ppo_minibatch_loss(clip_range_vf=...) clips against"""
    with torch.no_grad():
        return model.value(rollout["obs"]).flatten()


def ppo_minibatch_loss(model, rollout, prep, idx, clip_range=0.2, vf_coef=0.5, ent_coef=0.0, normalize_advantage=True, diagnostics=False,
                       clip_range_vf=None, old_values=None):
    """(loss, terms) of the rows idx of ppo_prepare's `prep`: the advantage normalised over the minibatch's used rows (unless switched
    off, or fewer than two are used), the surrogate clipped at clip_range, value loss and entropy.  terms: the rows' rho, log_ratio,
    a_hat, use, surr, value and policy_loss, value_loss, entropy, n_use; diagnostics: approx_kl and clip_fraction as well.
    clip_range_vf (None: off): stable-baselines3's value clipping - the value loss is taken on old_values + clamp(value - old_values,
    +- clip_range_vf), old_values [N] being ppo_old_values() at the start of the update."""
    adv, ret, old_logp, use = prep
    o, a = rollout["obs"].flatten(0, 1)[idx], rollout["action"].flatten(0, 1)[idx]
    u, a_hat = use[idx], adv[idx]
    n = u.sum()
    n_use = n.clamp(min=1.0)
    if normalize_advantage:
        mu = (a_hat * u).sum() / n_use
        sigma = ((((a_hat - mu) ** 2) * u).sum() / (n - 1.0).clamp(min=1.0)).sqrt()
        a_hat = torch.where(n > 1.0, (a_hat - mu) / (sigma + 1e-8), a_hat)
    log_ratio = model.dist(o).log_prob(a).sum(-1) - old_logp[idx]
    rho = log_ratio.exp()
    surr = torch.min(rho * a_hat, rho.clamp(1.0 - clip_range, 1.0 + clip_range) * a_hat)
    value = model.value(o)
    if clip_range_vf is None:
        value_pred = value
    else:
        if old_values is None:
            raise ValueError("clip_range_vf needs old_values (ppo_old_values at the start of the update)")
        value_pred = old_values[idx] + (value - old_values[idx]).clamp(-clip_range_vf, clip_range_vf)
    policy_loss, value_sum = -(surr * u).sum() / n_use, (((ret[idx] - value_pred) ** 2) * u).sum()
    loss, entropy = _entropy_term(model, policy_loss + vf_coef * value_sum / n_use, ent_coef)
    terms = {"policy_loss": policy_loss, "value_loss": value_sum / n_use, "entropy": entropy, "n_use": n_use, "rho": rho, "log_ratio": log_ratio,
             "a_hat": a_hat, "use": u, "surr": surr, "value": value}
    if diagnostics:
        with torch.no_grad():
            terms["approx_kl"] = (((rho - 1.0) - log_ratio) * u).sum() / n_use
            terms["clip_fraction"] = (((rho - 1.0).abs() > clip_range).to(u.dtype) * u).sum() / n_use
    return loss, terms


def ppo_update(model, opt, rollout, last_obs, n_epochs, batch_size, gamma=0.99, gae_lambda=0.95, clip_range=0.2, vf_coef=0.5, ent_coef=0.0,
               max_grad_norm=0.5, normalize_advantage=True, clip_range_vf=None, target_kl=None):
    """stable-baselines3's PPO.train() on one rollout: n_epochs passes over minibatches of batch_size rows, a torch.randperm from the
    global generator per pass.  clip_range_vf: ppo_minibatch_loss's.  target_kl (None: off): the update ends before the optimiser step
    of the first minibatch whose approx_kl exceeds 1.5 target_kl (one host read per minibatch, as in SB3).  Returns the number of
    optimiser steps applied."""
    prep = ppo_prepare(model, rollout, last_obs, gamma, gae_lambda)
    old_values = None if clip_range_vf is None else ppo_old_values(model, rollout)
    n_rows, applied = prep[0].numel(), 0
    for _ in range(n_epochs):
        perm = torch.randperm(n_rows, device=last_obs.device)
        for m in range(0, n_rows, batch_size):
            loss, terms = ppo_minibatch_loss(model, rollout, prep, perm[m:m + batch_size], clip_range, vf_coef, ent_coef, normalize_advantage,
                                             diagnostics=target_kl is not None, clip_range_vf=clip_range_vf, old_values=old_values)
            if target_kl is not None and float(terms["approx_kl"]) > 1.5 * target_kl:
                return applied
            optimizer_step(model, opt, loss, max_grad_norm)
            applied += 1
    return applied


def linear_schedule(initial):
    """progress_remaining (1 at the start of training, 0 at its end) -> progress_remaining * initial: stable-baselines3's usual schedule
    for lr and clip_range"""
    initial = float(initial)
    return lambda progress_remaining: progress_remaining * initial


class _TorchLearner:
    """the device learners' interface (`buffers`, `store`, `update`) around a torch optimiser `opt`, on the model's device"""

    def __init__(self, model, num_envs, n_steps, opt, **hyper):
        self.model, self.opt, self.hyper = model, opt, hyper
        self.buffers = rollout_buffers(n_steps, num_envs, model.pi[0].in_features, model.pi[-1].out_features, model.log_std.device)

    def store(self, k, obs, action, reward, done, resetting=None):
        store_rollout(self.buffers, k, obs, action, reward, done, resetting)

    def set_hyper(self, **kw):
        """rewrite hyper-parameters between updates: lr goes into the optimiser's param_groups, every other key into `hyper`"""
        for k, v in kw.items():
            if k == "lr":
                for g in self.opt.param_groups:
                    g["lr"] = v
            elif k in self.hyper:
                self.hyper[k] = v
            else:
                raise KeyError("%s has no hyper-parameter %r (it has lr, %s)" % (type(self).__name__, k, ", ".join(sorted(self.hyper))))


class TorchA2C(_TorchLearner):
    def __init__(self, model, num_envs, n_steps=5, gamma=0.99, lr=7e-4, alpha=0.99, eps=1e-5, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5):
        super().__init__(model, num_envs, n_steps, torch.optim.RMSprop(model.parameters(), lr=lr, alpha=alpha, eps=eps),
                         gamma=gamma, vf_coef=vf_coef, ent_coef=ent_coef, max_grad_norm=max_grad_norm)

    def update(self, last_obs):
        a2c_update(self.model, self.opt, self.buffers, last_obs, **self.hyper)


class TorchPPO(_TorchLearner):
    """batch_size None: ceil(N / 4)"""

    def __init__(self, model, num_envs, n_steps=16, n_epochs=4, batch_size=None, gamma=0.99, gae_lambda=0.95, clip_range=0.2, lr=3e-4,
                 betas=(0.9, 0.999), eps=1e-5, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5, normalize_advantage=True, clip_range_vf=None,
                 target_kl=None):
        super().__init__(model, num_envs, n_steps, torch.optim.Adam(model.parameters(), lr=lr, betas=betas, eps=eps),
                         n_epochs=n_epochs, batch_size=max(1, -(-n_steps * num_envs // 4)) if batch_size is None else int(batch_size), gamma=gamma,
                         gae_lambda=gae_lambda, clip_range=clip_range, vf_coef=vf_coef, ent_coef=ent_coef, max_grad_norm=max_grad_norm,
                         normalize_advantage=normalize_advantage, clip_range_vf=clip_range_vf, target_kl=target_kl)
        self._applied = 0

    def update(self, last_obs):
        self._applied = ppo_update(self.model, self.opt, self.buffers, last_obs, **self.hyper)

    def steps_applied(self):
        """optimiser steps the last update applied (fewer than n_epochs x minibatches when target_kl stopped it)"""
        return self._applied


def train(env_id="XarmReach-v0", num_envs=4096, updates=300, n_steps=None, gamma=0.99, lr=None, seed=0, config=None, log_every=50,
          quiet=False, auto_reset=True, log_dir=None, check_freq=1000, env=None, device_normalize=False, device_policy=False,
          device_update=False, algo="a2c", n_epochs=4, batch_size=None, gae_lambda=0.95, clip_range=0.2, net_arch=None, activation=None, wide=None,
          clip_range_vf=None, target_kl=None, shuffle=None, eval_freq=None, n_eval_episodes=None, eval_envs=None, eval_env=None, eval_graph=False):
    """auto_reset="lazy" (PickAndPlace): transitions flagged info["resetting"] carry no reward and no gradient and cut the
    return like an episode end - the env spends them on its reset ticks (include/xarm_hip.h XARM_AUTO_RESET_LAZY).
    log_dir: Monitor CSV + best-model checkpoints every `check_freq` env.step calls + the final VecNormalize statistics
    (benchmark/train.py:74,99,107-108).  env: an already built VecEnv (tests).
    device_normalize: normalisation and the Monitor in HIP kernels (gym_xarm_amd/normalize.py DeviceVecNormalize) instead of the
    torch classes of this file.
    device_policy: the rollout's sample and clamp in one HIP launch (gym_xarm_amd/device_policy.py DevicePolicy) instead of
    `model.dist(obs).sample().clamp(-1, 1)`; the update is unchanged and recomputes log-probabilities and values with autograd
    from the stored actions.
    device_update: the update itself - bootstrap value, returns, backward, clip_grad_norm_ and RMSprop - in HIP kernels on the
    model's own parameters (gym_xarm_amd/device_a2c.py DeviceA2C) instead of TorchA2C's a2c_update; no torch optimiser is created.
    algo: "a2c" (n_steps 5, lr 7e-4: the reference's learner) or "ppo" (n_steps 16, lr 3e-4): stable-baselines3's PPO.train() on each
    rollout (ppo_update) - GAE(gae_lambda) from the rollout's values, n_epochs passes over shuffled minibatches of batch_size rows (None:
    a quarter of the rollout), per-minibatch advantage normalisation over the used rows, the surrogate clipped at clip_range,
    clip_grad_norm_ and Adam(eps=1e-5).  With device_update the PPO update runs in HIP kernels too (gym_xarm_amd/device_ppo.py DevicePPO).
    net_arch / activation: ActorCritic's hidden widths and "tanh" / "relu" (None: 64-64 tanh), for either algo.  device_policy and the PPO
    device_update run equal widths of 64, 128, 192 or 256 units in two or three layers on their "wide" backends; the A2C
    device_update runs them on its "wide" backend when wide=True, and without it is the 64-64 tanh shape's and raises
    ValueError for any other.
    wide: handed to DeviceA2C / DevicePPO and to DevicePolicy as their `wide`; None leaves each class its default.
    clip_range_vf / target_kl (ppo; None: off): stable-baselines3's value clipping and early stop, in the torch block and in DevicePPO's
    kernels alike.  With target_kl the log records carry `ppo_steps_applied`, the optimiser steps the last update applied.
    lr, clip_range and clip_range_vf take a float or a callable of progress_remaining (linear_schedule): the learner is built with
    f(1) and `set_hyper` gets f(1 - it / updates) just before update `it` - where SB3 calls _update_current_progress_remaining, so a
    linear schedule runs its last update at 0.  A float is never passed through set_hyper.
    shuffle (ppo with device_update; None: "torch"): "torch" - torch.randperm per epoch - or "device" - DevicePPO's xarm_perm_fill, HIP launches
    inside the update call that allocate nothing and read nothing back.
    eval_freq (None: off, nothing is built): every eval_freq calls of env.step an evaluation.EvalCallback evaluates the deterministic policy
    with the normaliser's statistics frozen, for n_eval_episodes episodes (default: one per eval env) on `eval_env`, or on a second env of
    eval_envs (default min(num_envs, 1024)) envs made with seed + 1; it writes <log_dir>/evaluations.npz and best_eval_model.safetensors, the
    log records carry `eval_mean_reward` and `eval_success_rate` of the latest evaluation, and the callback is left on venv.eval_callback.
    eval_graph: the evaluator replays a captured iteration.
    Out of scope: schedules inside a captured graph (it holds the hyper-parameters of its capture), SAC schedules, use_sde."""
    if algo not in ("a2c", "ppo"):
        raise ValueError("algo must be 'a2c' or 'ppo'")
    ppo = algo == "ppo"
    n_steps = (16 if ppo else 5) if n_steps is None else n_steps
    lr = (3e-4 if ppo else 7e-4) if lr is None else lr
    torch.manual_seed(seed)
    if env is None:
        import gym_xarm_amd
        env = gym_xarm_amd.make(env_id, num_envs=num_envs, seed=seed, config=config, auto_reset=auto_reset)
    num_envs = env.num_envs
    dev = env.device
    if device_normalize:
        from .normalize import DeviceVecNormalize
        venv = DeviceVecNormalize(env, gamma=gamma, monitor_capacity=max(1 << 20, num_envs), log_dir=log_dir, env_id=env_id)
        monitor = venv.monitor                    # updated inside venv.step
    else:
        venv = VecNormalize(env, gamma=gamma)
        monitor = EpisodeMonitor(num_envs, dev, log_dir, env_id)
    callback = SaveOnBestTrainingRewardCallback(check_freq, log_dir, monitor, verbose=0 if quiet else 1) if log_dir else None
    eval_callback = None
    if eval_freq is not None:
        from .evaluation import make_eval_callback
        eval_callback = make_eval_callback(eval_freq, n_eval_episodes, eval_envs, eval_env, eval_graph, env_id, num_envs, seed, config, log_dir, quiet)
    model = ActorCritic(venv.dim, env.act_dim, (64, 64) if net_arch is None else tuple(net_arch), activation or "tanh").to(dev)
    n_rows = n_steps * num_envs
    batch_size = max(1, -(-n_rows // 4)) if batch_size is None else min(int(batch_size), n_rows)
    hyper = dict(n_steps=n_steps, gamma=gamma, lr=lr, eps=1e-5)
    if ppo:
        hyper.update(n_epochs=n_epochs, batch_size=batch_size, gae_lambda=gae_lambda, clip_range=clip_range)
        if clip_range_vf is not None or target_kl is not None:
            hyper.update(clip_range_vf=clip_range_vf, target_kl=target_kl)
    elif clip_range_vf is not None or target_kl is not None:
        raise ValueError("clip_range_vf and target_kl are PPO's (algo='ppo')")
    schedules = {k: f for k, f in hyper.items() if callable(f)}
    hyper.update({k: f(1.0) for k, f in schedules.items()})
    if device_update and "clip_range" in schedules and not schedules["clip_range"](0.0) > 0.0:
        raise ValueError("the device update needs clip_range > 0 at every update: this schedule gives %r at the last one (the torch block runs it)"
                         % (schedules["clip_range"](0.0),))
    if shuffle not in (None, "torch", "device"):
        raise ValueError("shuffle must be None, 'torch' or 'device', not %r" % (shuffle,))
    if shuffle == "device" and ppo and not device_update:
        raise ValueError("shuffle='device' is DevicePPO's (device_update=True); the torch update shuffles with torch.randperm")
    if device_update and ppo:
        from .device_ppo import DevicePPO
        learner = DevicePPO(model, num_envs, seed=seed, wide=wide, shuffle=shuffle or "torch", **hyper)
    elif device_update:
        from .device_a2c import DeviceA2C
        learner = DeviceA2C(model, num_envs, wide=wide, **hyper)
    else:
        learner = (TorchPPO if ppo else TorchA2C)(model, num_envs, **hyper)
    if device_policy:
        from .device_policy import DevicePolicy
        policy = DevicePolicy(model, seed=seed, row_offset=int(getattr(env, "_env_id_offset", 0)), wide=wide)
        env_action = torch.empty(num_envs, env.act_dim, device=dev)
    obs = venv.reset()
    hist, t0 = [], time.perf_counter()
    succ_sum, done_sum, raw_sum = torch.zeros((), device=dev), torch.zeros((), device=dev), torch.zeros((), device=dev)
    for it in range(1, updates + 1):
        for k in range(n_steps):
            if device_policy:
                # the sample lands in its slot of the rollout; env.step has read env_action when the next act_into rewrites it
                policy.act_into({"action": learner.buffers["action"][k], "env_action": env_action}, obs)
                a, a_env = None, env_action
            else:
                with torch.no_grad():
                    a = model.dist(obs).sample()
                a_env = a.clamp(-1, 1)
            nobs, nrew, done, info, raw = venv.step(a_env)
            resetting = info["resetting"] if "resetting" in info else None
            if not device_normalize:
                monitor.update(raw, done, None if resetting is None else ~resetting)
            if callback is not None:
                callback.on_step(model, venv, (it - 1) * n_steps * num_envs + (k + 1) * num_envs)
            if eval_callback is not None:
                eval_callback.on_step(model, venv, (it - 1) * n_steps * num_envs + (k + 1) * num_envs)
            learner.store(k, obs, a, nrew, done, resetting)
            succ_sum += (info["is_success"].float() * done.float()).sum()
            done_sum += done.float().sum()
            raw_sum += raw.mean()
            obs = nobs
        if schedules:
            learner.set_hyper(**{k: f(1.0 - it / updates) for k, f in schedules.items()})
        learner.update(obs)
        if it % log_every == 0 or it == updates:
            if dev.type == "cuda":
                torch.cuda.synchronize()
            rec = {"update": it, "env_steps": it * n_steps * num_envs, "mean_raw_reward": (raw_sum / (log_every * n_steps)).item(),
                   "success_rate": (succ_sum / done_sum.clamp(min=1)).item(), "episodes": int(done_sum.item()),
                   "env_steps_per_sec": it * n_steps * num_envs / (time.perf_counter() - t0)}
            if target_kl is not None:
                rec["ppo_steps_applied"] = learner.steps_applied()
            if eval_callback is not None and eval_callback.evaluations_timesteps:
                rec["eval_mean_reward"], rec["eval_success_rate"] = eval_callback.last_mean_reward, eval_callback.last_success_rate
            hist.append(rec)
            if not quiet:
                print(json.dumps(rec), flush=True)
            succ_sum.zero_(); done_sum.zero_(); raw_sum.zero_()
    monitor.flush()
    if log_dir:
        venv.save(os.path.join(log_dir, "vec_normalize.safetensors"))       # benchmark/train.py:107-108
    venv.monitor, venv.callback = monitor, callback
    if hasattr(torch.cuda, "synchronize") and dev.type == "cuda":
        torch.cuda.synchronize()
    if eval_callback is not None:
        venv.eval_callback = eval_callback
        eval_callback.eval_env.close()
    env.close()
    return model, venv, hist


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--env", default="XarmReach-v0")
    ap.add_argument("--num-envs", type=int, default=4096)
    ap.add_argument("--updates", type=int, default=300)
    ap.add_argument("--reward-type", default="dense")
    ap.add_argument("--save", default=None, help="safetensors file for the policy + VecNormalize statistics")
    ap.add_argument("--lazy-reset", action="store_true", help="opt-in lazy auto-reset (PickAndPlace), masked in the update")
    ap.add_argument("--log-dir", default=None, help="Monitor CSV, best_model.safetensors (every --check-freq calls), vec_normalize.safetensors")
    ap.add_argument("--check-freq", type=int, default=1000)
    ap.add_argument("--device-normalize", action="store_true", help="VecNormalize + Monitor in fused HIP kernels (gym_xarm_amd/normalize.py)")
    ap.add_argument("--device-policy", action="store_true", help="the rollout's sample + clamp in one HIP launch (gym_xarm_amd/device_policy.py)")
    ap.add_argument("--device-update", action="store_true", help="the update in HIP kernels (gym_xarm_amd/device_a2c.py, device_ppo.py, device_sac.py, device_td3.py)")
    ap.add_argument("--algo", choices=("a2c", "ppo", "sac", "td3"), default="a2c",
                    help="a2c: n-step returns, RMSprop; ppo: GAE, clipped surrogate, Adam; sac: SAC + HER (gym_xarm_amd/sac.py train_sac: --updates "
                         "counts env steps); td3: TD3 + HER (gym_xarm_amd/td3.py train_td3, likewise)")
    ap.add_argument("--n-steps", type=int, default=None, help="rollout length (a2c 5, ppo 16)")
    ap.add_argument("--n-epochs", type=int, default=4, help="ppo: passes over a rollout")
    ap.add_argument("--batch-size", type=int, default=None, help="ppo: rows per minibatch (default: a quarter of the rollout); sac: rows per step (256)")
    ap.add_argument("--gradient-steps", type=int, default=1, help="sac / td3: gradient steps per training env step")
    ap.add_argument("--policy-delay", type=int, default=None, help="td3: the actor and the targets step on every policy_delay-th gradient step (2)")
    ap.add_argument("--target-policy-noise", type=float, default=None, help="td3: standard deviation of the target policy smoothing noise (0.2)")
    ap.add_argument("--target-noise-clip", type=float, default=None, help="td3: clip of the smoothing noise (0.5)")
    ap.add_argument("--action-noise", type=float, default=None, help="td3: standard deviation of the Gaussian exploration noise (0.1)")
    ap.add_argument("--net-arch", type=int, nargs="+", default=None, help="hidden widths of every tower (default 64 64; the reference's sparse branch: 256 256 256)")
    ap.add_argument("--activation", choices=("tanh", "relu"), default=None, help="tanh (default) or relu (stable-baselines3's SAC default)")
    ap.add_argument("--wide", action="store_true", help="a2c / ppo: the per-layer GEMM chain for --device-update and --device-policy whatever the shape "
                                                        "(a2c: needed for any shape but 64 64 tanh)")
    ap.add_argument("--target-kl", type=float, default=None, help="ppo: stop an update before the first step whose approx_kl exceeds 1.5 x this")
    ap.add_argument("--clip-range-vf", type=float, default=None, help="ppo: clip the value's move from its call-start value to +- this")
    ap.add_argument("--lr-schedule", choices=("constant", "linear"), default="constant", help="a2c / ppo: linear runs lr down to 0 over --updates")
    ap.add_argument("--clip-range-schedule", choices=("constant", "linear"), default="constant", help="ppo: linear runs clip_range (0.2) down to 0")
    ap.add_argument("--shuffle", choices=("torch", "device"), default=None, help="ppo with --device-update: the minibatch shuffle (default torch; device: a HIP launch inside the update call)")
    ap.add_argument("--replay", choices=("her", "uniform"), default=None, help="sac / td3: the HER buffer, or stable-baselines3's plain ReplayBuffer "
                    "(gym_xarm_amd/replay.py; default: uniform on a flat-observation env, her otherwise)")
    ap.add_argument("--buffer-size", type=int, default=None, help="sac / td3 with the uniform buffer: transitions kept (1000000)")
    ap.add_argument("--eval-freq", type=int, default=None, help="evaluate the deterministic policy every this many env.step calls (gym_xarm_amd/evaluation.py "
                    "EvalCallback: evaluations.npz and best_eval_model.safetensors in --log-dir; default: off)")
    ap.add_argument("--eval-episodes", type=int, default=None, help="episodes per evaluation (default: one per eval env)")
    ap.add_argument("--eval-envs", type=int, default=None, help="envs of the evaluation env (default: min(--num-envs, 1024))")
    ap.add_argument("--eval-graph", action="store_true", help="the evaluator replays one captured iteration")
    args = ap.parse_args(argv)
    if args.eval_freq is None and (args.eval_episodes is not None or args.eval_envs is not None or args.eval_graph):
        ap.error("--eval-episodes, --eval-envs and --eval-graph need --eval-freq")
    evalkw = dict(eval_freq=args.eval_freq, n_eval_episodes=args.eval_episodes, eval_envs=args.eval_envs, eval_graph=args.eval_graph)
    if args.algo not in ("sac", "td3") and (args.replay is not None or args.buffer_size is not None):
        ap.error("--replay and --buffer-size are for --algo sac / td3")
    if args.algo != "ppo" and (args.target_kl is not None or args.clip_range_vf is not None or args.clip_range_schedule != "constant"):
        ap.error("--target-kl, --clip-range-vf and --clip-range-schedule are for --algo ppo")
    if args.algo in ("sac", "td3") and args.lr_schedule != "constant":
        ap.error("--lr-schedule is for --algo a2c / ppo")
    if args.algo != "td3" and any(v is not None for v in (args.policy_delay, args.target_policy_noise, args.target_noise_clip, args.action_noise)):
        ap.error("--policy-delay, --target-policy-noise, --target-noise-clip and --action-noise are for --algo td3")
    if args.algo != "ppo" and args.shuffle is not None:
        ap.error("--shuffle is for --algo ppo")
    if args.wide and args.algo == "sac":
        ap.error("--wide is for --algo a2c / ppo: the SAC device update selects its backend by shape")
    if args.wide and args.algo == "td3":
        ap.error("--wide is for --algo a2c / ppo: the TD3 device update has the per-layer GEMM chain only")
    cfg = {"reward_type": args.reward_type, "GUI": False} if ("Reach" in args.env or "PickAndPlace" in args.env) else None
    if "Handover" in args.env and "NoGoal" not in args.env:
        cfg = {"reward_type": args.reward_type}
    if args.algo == "sac":
        from . import sac
        model, venv, hist = sac.train_sac(args.env, num_envs=args.num_envs, steps=args.updates, batch_size=args.batch_size or 256,
                                          gradient_steps=args.gradient_steps, config=cfg, log_dir=args.log_dir, check_freq=args.check_freq,
                                          device_update=args.device_update, device_normalize=args.device_normalize,
                                          net_arch=None if args.net_arch is None else tuple(args.net_arch), activation=args.activation,
                                          replay=args.replay, buffer_size=args.buffer_size, **evalkw)
        if args.save:
            save_model(args.save, model, venv)
        return
    if args.algo == "td3":
        from . import td3
        extra = {k: v for k, v in (("policy_delay", args.policy_delay), ("target_policy_noise", args.target_policy_noise),
                                   ("target_noise_clip", args.target_noise_clip), ("action_noise", args.action_noise)) if v is not None}
        model, venv, hist = td3.train_td3(args.env, num_envs=args.num_envs, steps=args.updates, batch_size=args.batch_size or 256,
                                          gradient_steps=args.gradient_steps, config=cfg, log_dir=args.log_dir, check_freq=args.check_freq,
                                          device_update=args.device_update, device_normalize=args.device_normalize,
                                          net_arch=None if args.net_arch is None else tuple(args.net_arch), activation=args.activation,
                                          replay=args.replay, buffer_size=args.buffer_size, **extra, **evalkw)
        if args.save:
            save_model(args.save, model, venv)
        return
    model, venv, hist = train(args.env, args.num_envs, args.updates, config=cfg, auto_reset="lazy" if args.lazy_reset else True,
                              log_dir=args.log_dir, check_freq=args.check_freq, device_normalize=args.device_normalize,
                              device_policy=args.device_policy, device_update=args.device_update, algo=args.algo, n_steps=args.n_steps,
                              n_epochs=args.n_epochs, batch_size=args.batch_size, net_arch=None if args.net_arch is None else tuple(args.net_arch),
                              activation=args.activation, wide=True if args.wide else None, clip_range_vf=args.clip_range_vf, target_kl=args.target_kl,
                              lr=linear_schedule(3e-4 if args.algo == "ppo" else 7e-4) if args.lr_schedule == "linear" else None,
                              clip_range=linear_schedule(0.2) if args.clip_range_schedule == "linear" else 0.2, shuffle=args.shuffle, **evalkw)
    if args.save:
        save_model(args.save, model, venv)


if __name__ == "__main__":
    main()
