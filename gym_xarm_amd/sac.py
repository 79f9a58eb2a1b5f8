"""Soft actor-critic on the HER replay buffer - the off-policy learner of the reference's sparse-reward branch
(`benchmark/train.py`: `HerReplayBuffer`, learning_rate 1e-3, gamma 0.95, batch_size 256; `benchmark/display.py` loads the agent with
`SAC.load`).  SB3 itself is not installed here, so `SAC.train()` is written out in torch (`sac_step`), and `train_sac` is the driver:
it steps the batched env with the actor, stores every transition in a HER buffer (`DeviceHerReplayBuffer` on a GPU env,
`HerReplayBuffer` on a CPU env) and runs SAC steps on relabelled samples.  With `device_update` the action and the whole SAC step run in
HIP kernels on the module's own parameters (gym_xarm_amd/device_sac.py DeviceSAC); the torch block stays the default and
the checker.

The networks default to the project's 64-64 tanh shape (`policy_kwargs=dict(net_arch=[64, 64], activation_fn=nn.Tanh)` in SB3's terms);
`net_arch` and `activation` ("tanh" or "relu") build any other, the reference's `net_arch=[256, 256, 256]` with SB3's ReLU among them.  The
torch block runs every shape; the device update runs equal widths of 64, 128, 192 or 256 units in two or three hidden layers (DESIGN.md
24).  Out of scope: `use_sde`, `n_critics != 2`.

  python -m gym_xarm_amd.train --algo sac --env XarmReach-v0 --num-envs 256 --updates 2000 --reward-type sparse --device-update
"""
import copy
import json
import math
import os
import time

import torch
import torch.nn as nn

from .replay import UNIFORM_BUFFERS

LOG_STD_MIN, LOG_STD_MAX, SQUASH_EPS = -20.0, 2.0, 1e-6


ACTIVATIONS = {"tanh": nn.Tanh, "relu": nn.ReLU}


def _tower(n_in, n_out, net_arch=(64, 64), activation="tanh"):
    layers, last = [], n_in
    for width in net_arch:
        layers += [nn.Linear(last, width), ACTIVATIONS[activation]()]
        last = width
    return nn.Sequential(*layers, nn.Linear(last, n_out))


class SacPolicy(nn.Module):
    """SB3's SAC 'MlpPolicy': a squashed-Gaussian actor D -> net_arch -> 2A (rows 0 .. A-1 of the last layer the mean, A .. 2A-1
    log_std), two critics and their targets D + A -> net_arch -> 1, and log_alpha.  net_arch: the hidden widths (default (64, 64));
    activation: "tanh" (default) or "relu" (SB3's own default for SAC).  Both are kept as attributes."""

    def __init__(self, obs_dim, act_dim, net_arch=(64, 64), activation="tanh"):
        super().__init__()
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.net_arch, self.activation = tuple(int(n) for n in net_arch), str(activation)
        if not self.net_arch or min(self.net_arch) < 1:
            raise ValueError("net_arch must name at least one hidden layer of at least one unit")
        if self.activation not in ACTIVATIONS:
            raise ValueError("activation must be 'tanh' or 'relu', not %r" % (activation,))
        tower = lambda n_in, n_out: _tower(n_in, n_out, self.net_arch, self.activation)
        self.actor = tower(obs_dim, 2 * act_dim)
        self.q1, self.q2 = tower(obs_dim + act_dim, 1), tower(obs_dim + act_dim, 1)
        self.q1_target, self.q2_target = copy.deepcopy(self.q1), copy.deepcopy(self.q2)
        for p in list(self.q1_target.parameters()) + list(self.q2_target.parameters()):
            p.requires_grad_(False)
        self.log_alpha = nn.Parameter(torch.zeros(1))

    def action_log_prob(self, obs, z=None, deterministic=False):
        """(a, logp): u = mean + exp(clamp(log_std, -20, 2)) z, a = tanh(u),
        logp = sum(-z^2 / 2 - log_std - log(2 pi) / 2) - sum(log(1 - a^2 + 1e-6)).  z None: drawn here."""
        out = self.actor(obs)
        A = self.act_dim
        mean, log_std = out[..., :A], out[..., A:].clamp(LOG_STD_MIN, LOG_STD_MAX)
        if deterministic:
            z = torch.zeros_like(mean)
        elif z is None:
            z = torch.randn_like(mean)
        a = torch.tanh(mean + log_std.exp() * z)
        logp = (-0.5 * z * z - log_std - 0.5 * math.log(2.0 * math.pi)).sum(-1) - torch.log(1.0 - a * a + SQUASH_EPS).sum(-1)
        return a, logp

    def q_values(self, obs, action, target=False):
        x = torch.cat([obs, action], dim=-1)
        q1, q2 = (self.q1_target, self.q2_target) if target else (self.q1, self.q2)
        return q1(x).squeeze(-1), q2(x).squeeze(-1)

    def critic_parameters(self):
        return list(self.q1.parameters()) + list(self.q2.parameters())


def make_optimizers(model, lr=1e-3, ent_coef="auto", betas=(0.9, 0.999), eps=1e-8):
    """the torch block's three Adams: actor, both critics, log_alpha (None with a fixed ent_coef)"""
    kw = dict(lr=lr, betas=betas, eps=eps)
    return {"actor": torch.optim.Adam(model.actor.parameters(), **kw), "critic": torch.optim.Adam(model.critic_parameters(), **kw),
            "alpha": torch.optim.Adam([model.log_alpha], **kw) if ent_coef == "auto" else None}


def sac_step(model, opts, batch, gamma=0.95, tau=0.005, ent_coef="auto", target_entropy=None, z_pi=None, z_next=None):
    """One gradient step of SB3's SAC.train() on `batch` (obs, next_obs [B, D] normalised, action [B, A], reward, done [B], optional
    use [B]: every mean is over the rows with use = 1).  Returns the step's stats as a dict of 0-d tensors."""
    obs, nobs, act, rew = batch["obs"], batch["next_obs"], batch["action"], batch["reward"]
    done = batch["done"].to(rew.dtype)
    use = batch.get("use")
    use = torch.ones_like(rew) if use is None else use.to(rew.dtype)
    n_use = use.sum().clamp(min=1.0)
    mean = lambda x: (x * use).sum() / n_use
    te = -float(model.act_dim) if target_entropy is None else float(target_entropy)
    a_pi, logp_pi = model.action_log_prob(obs, z_pi)
    if ent_coef == "auto":
        alpha = model.log_alpha.detach().exp().squeeze()
        alpha_loss = -mean(model.log_alpha.squeeze() * (logp_pi.detach() + te))
        opts["alpha"].zero_grad(set_to_none=True)
        alpha_loss.backward()
        opts["alpha"].step()
    else:
        alpha, alpha_loss = torch.as_tensor(float(ent_coef), dtype=rew.dtype, device=rew.device), torch.zeros((), dtype=rew.dtype, device=rew.device)
    with torch.no_grad():
        a_next, logp_next = model.action_log_prob(nobs, z_next)
        q1t, q2t = model.q_values(nobs, a_next, target=True)
        y = rew + gamma * (1.0 - done) * (torch.minimum(q1t, q2t) - alpha * logp_next)
    q1, q2 = model.q_values(obs, act)
    critic_loss = 0.5 * (mean((q1 - y) ** 2) + mean((q2 - y) ** 2))
    opts["critic"].zero_grad(set_to_none=True)
    critic_loss.backward()
    opts["critic"].step()
    q1p, q2p = model.q_values(obs, a_pi)
    qmin = torch.minimum(q1p, q2p)
    actor_loss = mean(alpha * logp_pi - qmin)
    opts["actor"].zero_grad(set_to_none=True)
    actor_loss.backward()
    opts["actor"].step()
    with torch.no_grad():
        for t, c in zip(list(model.q1_target.parameters()) + list(model.q2_target.parameters()), model.critic_parameters()):
            t.mul_(1.0 - tau).add_(c, alpha=tau)
    d = lambda x: x.detach()
    return {"critic_loss": d(critic_loss), "actor_loss": d(actor_loss), "alpha_loss": d(alpha_loss), "alpha": d(alpha), "logp_pi": d(mean(logp_pi)),
            "min_q": d(mean(qmin)), "n_use": d(n_use)}


STATS = ("critic_loss", "actor_loss", "alpha_loss", "alpha", "logp_pi", "min_q", "n_use")


def _frozen_norm(venv, x):
    """clamp((x - mean) / sqrt(var + eps), +-clip_obs) with the wrapper's statistics as they are (VecNormalize or DeviceVecNormalize)"""
    if hasattr(venv, "stats"):      # DeviceVecNormalize: float64 statistics, one rounding to float32 as its kernels do
        y = ((x.double() - venv.obs_mean) / torch.sqrt(venv.obs_var + venv.eps)).clamp(-venv.clip_obs, venv.clip_obs)
        return y.float()
    return ((x - venv.obs_rms.mean) / torch.sqrt(venv.obs_rms.var + venv.eps)).clamp(-venv.clip_obs, venv.clip_obs)


def normalized_batch(venv, s):
    """the SAC batch of a HER sample `s`: both observation triples concatenated and normalised with the running statistics as they
    are now, raw rewards, `ok` (where the buffer has it) as use"""
    cat = lambda *k: torch.cat([s[x] for x in k], dim=1)
    b = {"obs": _frozen_norm(venv, cat("observation", "achieved_goal", "desired_goal")),
         "next_obs": _frozen_norm(venv, cat("next_observation", "next_achieved_goal", "desired_goal")),
         "action": s["action"], "reward": s["reward"], "done": s["done"].float()}
    if "ok" in s:
        b["use"] = s["ok"].float()
    return b


def flat_batch(venv, s):
    """the learner's batch of a uniform-replay sample `s` (replay.ReplayBuffer.sample): both observation rows normalised with the running
    statistics as they are now, raw rewards, done with the time-limit truncations already taken out - normalized_batch's counterpart"""
    return {"obs": _frozen_norm(venv, s["obs"]), "next_obs": _frozen_norm(venv, s["next_obs"]), "action": s["action"], "reward": s["reward"],
            "done": s["done"].float(), "use": s["use"].float()}


def train_off_policy(build, stats, env_id="XarmReach-v0", num_envs=256, steps=2000, batch_size=256, gradient_steps=1, train_freq=1, learning_starts=None,
                     gamma=0.95, n_sampled_goal=4, goal_selection_strategy="future", seed=0, env=None, log_dir=None, device_normalize=False, config=None,
                     log_every=50, quiet=False, check_freq=1000, horizon=None, replay=None, buffer_size=None, eval_freq=None, n_eval_episodes=None,
                     eval_envs=None, eval_env=None, eval_graph=False):
    """The driver loop that `train_sac` and `td3.train_td3` share: an off-policy learner on a batched env, with HER on a goal env
    (replay="her") or SB3's plain uniform buffer (replay="uniform": gym_xarm_amd/replay.py; the flat-observation env, or a goal env
    without relabelling; buffer_size: its transitions, default 1 000 000).  replay=None: "uniform" on a flat-observation env, else "her".
    The uniform buffer is told which finished envs ran into the time limit (info["TimeLimit.truncated"]) and samples those transitions
    with done = 0; the HER buffer stores them as terminations.  The driver builds the env, the normaliser, the Monitor, the callback
    and the buffer, then calls `build(venv, env, buffer, dev, num_envs, act_dim, learning_starts)`
    -> (model, act, learn): `act(nobs, it)` is the rollout action [E, A] of step `it`, `learn()` samples the buffer and runs one gradient step,
    returning its stats (a tensor in the order of `stats`, or a dict of 0-d tensors keyed by it).  eval_freq, n_eval_episodes, eval_envs,
    eval_env, eval_graph: train.train's - the deterministic action on a second env (evaluation.EvalCallback, left on venv.eval_callback),
    `eval_mean_reward` and `eval_success_rate` in the log records; None builds nothing.  Returns (model, venv, hist)."""
    from .her import DeviceHerReplayBuffer, HerReplayBuffer
    from .replay import DeviceReplayBuffer, ReplayBuffer
    from .train import EpisodeMonitor, SaveOnBestTrainingRewardCallback, VecNormalize
    torch.manual_seed(seed)
    if env is None:
        import gym_xarm_amd
        env = gym_xarm_amd.make(env_id, num_envs=num_envs, seed=seed, config=config, auto_reset=True)
    assert not getattr(env, "_lazy", False), "the off-policy driver stores terminal observations: it needs the in-call auto-reset (auto_reset=True)"
    num_envs, dev = env.num_envs, torch.device(env.device)
    flat = bool(getattr(env, "flat_observation", False))
    replay = ("uniform" if flat else "her") if replay is None else replay
    if replay not in ("her", "uniform"):
        raise ValueError("replay must be 'her' or 'uniform', not %r" % (replay,))
    if replay == "her" and flat:
        raise ValueError("replay='her' needs a goal env: a flat-observation env has no achieved or desired goal to relabel (use replay='uniform')")
    uniform = replay == "uniform"
    act_dim = int(getattr(env, "action_dim", getattr(env, "act_dim", 0)))
    max_len = int(getattr(env, "max_episode_steps", 50))
    learning_starts = 2 * max_len if learning_starts is None else int(learning_starts)
    if device_normalize:
        from .normalize import DeviceVecNormalize
        venv = DeviceVecNormalize(env, gamma=gamma, monitor_capacity=max(1 << 20, num_envs), log_dir=log_dir, env_id=env_id)
        monitor = venv.monitor
        norm_out = venv.alloc_out()
    else:
        venv = VecNormalize(env, gamma=gamma)
        monitor = EpisodeMonitor(num_envs, dev, log_dir, env_id)
    callback = SaveOnBestTrainingRewardCallback(check_freq, log_dir, monitor, verbose=0 if quiet else 1) if log_dir else None
    if uniform:
        Buffer = DeviceReplayBuffer if dev.type == "cuda" else ReplayBuffer
        buffer = Buffer(env, buffer_size=1_000_000 if buffer_size is None else int(buffer_size), seed=seed)
    else:
        Buffer = DeviceHerReplayBuffer if dev.type == "cuda" else HerReplayBuffer
        buffer = Buffer(env, horizon=horizon, n_sampled_goal=n_sampled_goal, goal_selection_strategy=goal_selection_strategy, seed=seed)
    model, act, learn = build(venv, env, buffer, dev, num_envs, act_dim, learning_starts)
    eval_callback = None
    if eval_freq is not None:
        from .evaluation import make_eval_callback
        eval_callback = make_eval_callback(eval_freq, n_eval_episodes, eval_envs, eval_env, eval_graph, env_id, num_envs, seed, config, log_dir, quiet)
    obs = env.reset()
    nobs = venv.reset_from(obs) if device_normalize else venv._norm(venv._flat(obs))
    hist, t0, last, updates, window = [], time.perf_counter(), None, 0, 0
    succ_sum, done_sum, raw_sum = torch.zeros((), device=dev), torch.zeros((), device=dev), torch.zeros((), device=dev)
    for it in range(1, steps + 1):
        prev = obs.clone() if flat else {k: v.clone() for k, v in obs.items()}
        a = act(nobs, it)
        obs, rew, done, info = env.step(a)
        term = info.get("terminal_observation")
        if term is None:
            nxt = obs
        elif flat:          # the terminal observation is the row itself
            nxt = torch.where((done != 0)[:, None], term, obs)
        else:
            d = (done != 0)[:, None]
            nxt = {"observation": torch.where(d, term, obs["observation"]), "achieved_goal": torch.where(d, env.achieved_goal_of(term), obs["achieved_goal"])}
        if uniform:
            buffer.add(prev, nxt, a, rew, done, info.get("TimeLimit.truncated"))
        else:
            buffer.add(prev, nxt, a, rew, done)
        if device_normalize:
            nobs = venv.step_into(norm_out, obs, rew, done)["nobs"]
        else:
            nobs = venv._norm(venv._flat(obs))
            monitor.update(rew, done)
        if callback is not None:
            callback.on_step(model, venv, it * num_envs)
        if eval_callback is not None:
            eval_callback.on_step(model, venv, it * num_envs)
        if it > learning_starts and it % train_freq == 0:
            for _ in range(gradient_steps):
                last = learn()
                updates += 1
        succ_sum += (info["is_success"].float() * done.float()).sum()
        done_sum += done.float().sum()
        raw_sum += rew.mean()
        window += 1
        if it % log_every == 0 or it == steps:
            if dev.type == "cuda":
                torch.cuda.synchronize()
            rec = {"step": it, "env_steps": it * num_envs, "updates": updates, "mean_raw_reward": (raw_sum / window).item(),
                   "success_rate": (succ_sum / done_sum.clamp(min=1)).item(), "episodes": int(done_sum.item()),
                   "env_steps_per_sec": it * num_envs / (time.perf_counter() - t0)}
            if last is not None:
                vals = last.tolist() if torch.is_tensor(last) else [float(last[k]) for k in stats]
                rec.update({k: float(v) for k, v in zip(stats, vals)})
            if eval_callback is not None and eval_callback.evaluations_timesteps:
                rec["eval_mean_reward"], rec["eval_success_rate"] = eval_callback.last_mean_reward, eval_callback.last_success_rate
            hist.append(rec)
            if not quiet:
                print(json.dumps(rec), flush=True)
            succ_sum.zero_(); done_sum.zero_(); raw_sum.zero_()
            window = 0
    monitor.flush()
    if log_dir:
        venv.save(os.path.join(log_dir, "vec_normalize.safetensors"))
    venv.monitor, venv.callback, venv.buffer = monitor, callback, buffer
    if dev.type == "cuda":
        torch.cuda.synchronize()
    if eval_callback is not None:
        venv.eval_callback = eval_callback
        eval_callback.eval_env.close()
    env.close()
    return model, venv, hist


def train_sac(env_id="XarmReach-v0", num_envs=256, steps=2000, batch_size=256, gradient_steps=1, train_freq=1, learning_starts=None, gamma=0.95,
              lr=1e-3, tau=0.005, ent_coef="auto", target_entropy=None, n_sampled_goal=4, goal_selection_strategy="future", seed=0, env=None,
              log_dir=None, device_update=False, device_normalize=False, config=None, log_every=50, quiet=False, check_freq=1000, horizon=None,
              net_arch=None, activation=None, replay=None, buffer_size=None, eval_freq=None, n_eval_episodes=None, eval_envs=None, eval_env=None,
              eval_graph=False):
    """SAC + HER on a batched goal env, or - replay="uniform", the default on a flat-observation env such as XarmPDHandoverNoGoal-v1 - SAC on
    SB3's plain ReplayBuffer of `buffer_size` transitions (default 1 000 000), which bootstraps through time-limit truncations; "uniform" on
    a goal env is the dense-reward / no-relabel setting.  steps: calls of env.step (num_envs transitions each).  After `learning_starts` steps (default
    2 x max_episode_steps, so that closed episodes exist) every `train_freq`-th step runs `gradient_steps` SAC steps on `batch_size`
    relabelled rows.  Observations are normalised at sample time with the running statistics; rewards stay raw.
    device_update: the rollout action and the SAC step in HIP kernels (DeviceSAC).  device_normalize: DeviceVecNormalize (statistics,
    Monitor and - with device_update - the sample's normalisation in HIP kernels); with both on a GPU env an iteration reads nothing
    back outside logging.  log_dir, check_freq: Monitor CSV, best-model checkpoints and the final statistics as in train().
    net_arch, activation: SacPolicy's (None: 64-64 tanh); a best-model checkpoint of another shape carries both beside the state_dict
    (`load_checkpoint` rebuilds the module).  eval_freq, n_eval_episodes, eval_envs, eval_env, eval_graph: train_off_policy's.  The loop itself is `train_off_policy`, shared with td3.train_td3.
    Returns (model, venv, hist)."""
    def build(venv, env, buffer, dev, num_envs, act_dim, learning_starts):
        model = SacPolicy(venv.dim, act_dim, (64, 64) if net_arch is None else net_arch, "tanh" if activation is None else activation).to(dev)
        if device_update:
            from .device_sac import DeviceSAC
            dsac = DeviceSAC(model, batch_size, gamma=gamma, lr=lr, tau=tau, ent_coef=ent_coef, target_entropy=target_entropy, seed=seed,
                             row_offset=int(getattr(env, "_env_id_offset", 0)), act_rows=num_envs)
            act_out = {"action": torch.empty(num_envs, act_dim, device=dev)}
            sample = buffer.alloc_out(batch_size)
            act = lambda nobs, it: dsac.act_into(act_out, nobs)["action"]
            to_batch = flat_batch if isinstance(buffer, UNIFORM_BUFFERS) else normalized_batch
            if device_normalize:
                learn = lambda: dsac.update_from(buffer, venv, sample)
            else:
                learn = lambda: dsac.update(to_batch(venv, buffer.sample_into(sample)))
        else:
            opts = make_optimizers(model, lr, ent_coef)

            def act(nobs, it):
                with torch.no_grad():
                    return model.action_log_prob(nobs)[0]
            to_batch = flat_batch if isinstance(buffer, UNIFORM_BUFFERS) else normalized_batch
            learn = lambda: sac_step(model, opts, to_batch(venv, buffer.sample(batch_size)), gamma, tau, ent_coef, target_entropy)
        return model, act, learn
    return train_off_policy(build, STATS, env_id=env_id, num_envs=num_envs, steps=steps, batch_size=batch_size, gradient_steps=gradient_steps,
                            train_freq=train_freq, learning_starts=learning_starts, gamma=gamma, n_sampled_goal=n_sampled_goal,
                            goal_selection_strategy=goal_selection_strategy, seed=seed, env=env, log_dir=log_dir, device_normalize=device_normalize,
                            config=config, log_every=log_every, quiet=quiet, check_freq=check_freq, horizon=horizon, replay=replay,
                            buffer_size=buffer_size, eval_freq=eval_freq, n_eval_episodes=n_eval_episodes, eval_envs=eval_envs, eval_env=eval_env,
                            eval_graph=eval_graph)


def load_checkpoint(path):
    """(SacPolicy, vecnormalize state) of a checkpoint written by train_sac (`best_model.safetensors`, train.save_model): the tensors are
    `policy.<state_dict key>` and `vecnormalize.<key>`; the file's metadata holds `net_arch` ("256,256,256") and `activation`, from which
    the module is rebuilt before its state_dict is loaded (a file without them is the 64-64 tanh shape); obs_dim and act_dim are read off
    the actor's first and last layer"""
    from safetensors import safe_open
    from safetensors.torch import load_file
    with safe_open(path, framework="pt") as f:
        meta = f.metadata() or {}
    sd = load_file(path)
    pol = {k[len("policy."):]: v for k, v in sd.items() if k.startswith("policy.")}
    arch = tuple(int(n) for n in meta["net_arch"].split(",")) if "net_arch" in meta else (64, 64)
    model = SacPolicy(pol["actor.0.weight"].shape[1], pol["actor.%d.bias" % (2 * len(arch))].shape[0] // 2, arch, meta.get("activation", "tanh"))
    model.load_state_dict(pol)
    return model, {k[len("vecnormalize."):]: v for k, v in sd.items() if k.startswith("vecnormalize.")}
