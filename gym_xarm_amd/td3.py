"""Twin delayed DDPG on the HER replay buffer - the other stable-baselines3 learner that runs on `HerReplayBuffer` with continuous
actions, beside gym_xarm_amd/sac.py's SAC (the reference's sparse-reward branch: learning_rate 1e-3, gamma 0.95, batch_size 256,
`net_arch=[256, 256, 256]`).  SB3 itself is not installed here, so `TD3.train()` is written out in torch (`td3_step`), and `train_td3`
is the driver: sac.train_off_policy's loop with TD3's exploration and step.  With `device_update` the action and the whole TD3 step run
in HIP kernels on the module's own parameters (gym_xarm_amd/device_td3.py DeviceTD3); the torch block stays the default
and the checker.

The networks default to the project's 64-64 tanh shape; `net_arch` and `activation` ("tanh" or "relu") build any other.  The torch block
runs every shape; the device update runs equal widths of 64, 128, 192 or 256 units in two or three hidden layers.  Out of scope: DDPG and
`n_critics != 2`, `use_sde`, schedules, `train_freq` tuples.

  python -m gym_xarm_amd.train --algo td3 --env XarmReach-v0 --num-envs 256 --updates 2000 --reward-type sparse --device-update
"""
import copy

import torch
import torch.nn as nn

from . import sac
from .sac import normalized_batch

STATS = ("critic_loss", "actor_loss", "q1_pi", "target_q", "n_use", "actor_stepped")


class Td3Policy(nn.Module):
    """SB3's TD3 'MlpPolicy': a deterministic actor D -> net_arch -> A with tanh on the output, two critics D + A -> net_arch -> 1, and a
    target of each of the three (deep copies that take no gradient).  net_arch: the hidden widths (default (64, 64)); activation: "tanh"
    (default) or "relu".  Both are kept as attributes; `algo` = "td3" goes into a checkpoint's metadata.  SB3's own default is [400, 300]
    with ReLU: unequal widths, which run on the torch block (`td3_step`) only - the device update needs equal widths."""

    algo = "td3"

    def __init__(self, obs_dim, act_dim, net_arch=(64, 64), activation="tanh"):
        super().__init__()
        self.obs_dim, self.act_dim = int(obs_dim), int(act_dim)
        self.net_arch, self.activation = tuple(int(n) for n in net_arch), str(activation)
        if not self.net_arch or min(self.net_arch) < 1:
            raise ValueError("net_arch must name at least one hidden layer of at least one unit")
        if self.activation not in sac.ACTIVATIONS:
            raise ValueError("activation must be 'tanh' or 'relu', not %r" % (activation,))
        tower = lambda n_in, n_out: sac._tower(n_in, n_out, self.net_arch, self.activation)
        self.actor = tower(obs_dim, act_dim)
        self.q1, self.q2 = tower(obs_dim + act_dim, 1), tower(obs_dim + act_dim, 1)
        self.actor_target, self.q1_target, self.q2_target = copy.deepcopy(self.actor), copy.deepcopy(self.q1), copy.deepcopy(self.q2)
        for p in self.target_parameters():
            p.requires_grad_(False)

    def action(self, obs, target=False):
        return torch.tanh((self.actor_target if target else self.actor)(obs))

    def q_values(self, obs, action, target=False):
        x = torch.cat([obs, action], dim=-1)
        q1, q2 = (self.q1_target, self.q2_target) if target else (self.q1, self.q2)
        return q1(x).squeeze(-1), q2(x).squeeze(-1)

    def critic_parameters(self):
        return list(self.q1.parameters()) + list(self.q2.parameters())

    def target_parameters(self):
        return list(self.actor_target.parameters()) + list(self.q1_target.parameters()) + list(self.q2_target.parameters())


def make_optimizers(model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """the torch block's two Adams: actor, both critics"""
    kw = dict(lr=lr, betas=betas, eps=eps)
    return {"actor": torch.optim.Adam(model.actor.parameters(), **kw), "critic": torch.optim.Adam(model.critic_parameters(), **kw)}


def td3_step(model, opts, batch, n_updates, gamma=0.95, tau=0.005, policy_delay=2, target_policy_noise=0.2, target_noise_clip=0.5, z_next=None,
             last=None):
    """One gradient step of SB3's TD3.train() on `batch` (obs, next_obs [B, D] normalised, action [B, A], reward, done [B], optional
    use [B]: every mean is over the rows with use = 1).  n_updates: the gradient steps so far, counted from 1 and including this one; the
    actor and the three targets step when n_updates % policy_delay == 0.  z_next [B, A]: the smoothing noise's standard normals (drawn
    here when None).  Returns the step's stats as a dict of 0-d tensors (STATS); on a step without an actor update actor_loss and q1_pi
    repeat `last`'s (the previous step's dict; zeros when None)."""
    obs, nobs, act, rew = batch["obs"], batch["next_obs"], batch["action"], batch["reward"]
    done = batch["done"].to(rew.dtype)
    use = batch.get("use")
    use = torch.ones_like(rew) if use is None else use.to(rew.dtype)
    n_use = use.sum().clamp(min=1.0)
    mean = lambda x: (x * use).sum() / n_use
    with torch.no_grad():
        z = torch.randn_like(act) if z_next is None else z_next
        noise = (target_policy_noise * z).clamp(-target_noise_clip, target_noise_clip)
        a_next = (model.action(nobs, target=True) + noise).clamp(-1.0, 1.0)
        q1t, q2t = model.q_values(nobs, a_next, target=True)
        y = rew + (1.0 - done) * gamma * torch.minimum(q1t, q2t)
    q1, q2 = model.q_values(obs, act)
    critic_loss = mean((q1 - y) ** 2) + mean((q2 - y) ** 2)
    opts["critic"].zero_grad(set_to_none=True)
    critic_loss.backward()
    opts["critic"].step()
    zero = torch.zeros((), dtype=rew.dtype, device=rew.device)
    stepped = n_updates % policy_delay == 0
    if stepped:
        q1_pi = mean(model.q_values(obs, model.action(obs))[0])
        actor_loss = -q1_pi
        opts["actor"].zero_grad(set_to_none=True)
        actor_loss.backward()
        opts["actor"].step()
        with torch.no_grad():
            for t, c in zip(model.target_parameters(), list(model.actor.parameters()) + model.critic_parameters()):
                t.mul_(1.0 - tau).add_(c, alpha=tau)
    else:
        actor_loss, q1_pi = (zero, zero) if last is None else (last["actor_loss"], last["q1_pi"])
    d = lambda x: x.detach()
    return {"critic_loss": d(critic_loss), "actor_loss": d(actor_loss), "q1_pi": d(q1_pi), "target_q": d(mean(y)), "n_use": d(n_use),
            "actor_stepped": zero + float(stepped)}


def train_td3(env_id="XarmReach-v0", num_envs=256, steps=2000, batch_size=256, gradient_steps=1, train_freq=1, learning_starts=None, gamma=0.95,
              lr=1e-3, tau=0.005, policy_delay=2, target_policy_noise=0.2, target_noise_clip=0.5, action_noise=0.1, n_sampled_goal=4,
              goal_selection_strategy="future", seed=0, env=None, log_dir=None, device_update=False, device_normalize=False, config=None,
              log_every=50, quiet=False, check_freq=1000, horizon=None, net_arch=None, activation=None, replay=None, buffer_size=None,
              eval_freq=None, n_eval_episodes=None, eval_envs=None, eval_env=None, eval_graph=False):
    """TD3 + HER on a batched goal env, or TD3 on the uniform buffer (replay, buffer_size: as in sac.train_sac): sac.train_sac's arguments
    without the entropy coefficient's, plus TD3's.  Exploration is SB3's
    `_sample_action`: uniform actions in [-1, 1] while the step count is <= learning_starts, after that
    clamp(actor(nobs) + action_noise z, -1, 1); the stored action is the clamped one.  device_update: the rollout action and the TD3 step in
    HIP kernels (DeviceTD3); device_normalize: DeviceVecNormalize, as in train_sac.  eval_freq, n_eval_episodes, eval_envs, eval_env,
    eval_graph: sac.train_off_policy's.  Returns (model, venv, hist)."""
    def build(venv, env, buffer, dev, num_envs, act_dim, learning_starts):
        model = Td3Policy(venv.dim, act_dim, (64, 64) if net_arch is None else net_arch, "tanh" if activation is None else activation).to(dev)
        if device_update:
            from .device_td3 import DeviceTD3
            dtd3 = DeviceTD3(model, batch_size, gamma=gamma, lr=lr, tau=tau, policy_delay=policy_delay, target_policy_noise=target_policy_noise,
                             target_noise_clip=target_noise_clip, action_noise=action_noise, seed=seed,
                             row_offset=int(getattr(env, "_env_id_offset", 0)), act_rows=num_envs)
            act_out = torch.empty(num_envs, act_dim, device=dev)
            sample = buffer.alloc_out(batch_size)
            act = lambda nobs, it: dtd3.act_into(act_out, nobs, "uniform" if it <= learning_starts else "gaussian")
            to_batch = sac.flat_batch if isinstance(buffer, sac.UNIFORM_BUFFERS) else normalized_batch
            if device_normalize:
                learn = lambda: dtd3.update_from(buffer, venv, sample)
            else:
                learn = lambda: dtd3.update(to_batch(venv, buffer.sample_into(sample)))
        else:
            opts = make_optimizers(model, lr)
            state = {"n": 0, "last": None}
            to_batch = sac.flat_batch if isinstance(buffer, sac.UNIFORM_BUFFERS) else normalized_batch

            def act(nobs, it):
                with torch.no_grad():
                    if it <= learning_starts:
                        return torch.rand(num_envs, act_dim, device=dev) * 2.0 - 1.0
                    a = model.action(nobs)
                    return (a + action_noise * torch.randn_like(a)).clamp(-1.0, 1.0)

            def learn():
                state["n"] += 1
                state["last"] = td3_step(model, opts, to_batch(venv, buffer.sample(batch_size)), state["n"], gamma, tau, policy_delay,
                                         target_policy_noise, target_noise_clip, last=state["last"])
                return state["last"]
        return model, act, learn
    return sac.train_off_policy(build, STATS, env_id=env_id, num_envs=num_envs, steps=steps, batch_size=batch_size, gradient_steps=gradient_steps,
                                train_freq=train_freq, learning_starts=learning_starts, gamma=gamma, n_sampled_goal=n_sampled_goal,
                                goal_selection_strategy=goal_selection_strategy, seed=seed, env=env, log_dir=log_dir,
                                device_normalize=device_normalize, config=config, log_every=log_every, quiet=quiet, check_freq=check_freq,
                                horizon=horizon, replay=replay, buffer_size=buffer_size, eval_freq=eval_freq, n_eval_episodes=n_eval_episodes,
                                eval_envs=eval_envs, eval_env=eval_env, eval_graph=eval_graph)


def load_checkpoint(path):
    """(Td3Policy, vecnormalize state) of a checkpoint written by train_td3 (`best_model.safetensors`, train.save_model), as
    sac.load_checkpoint: the metadata holds `net_arch`, `activation` and `algo` = "td3" (a file that names another algo is refused)"""
    from safetensors import safe_open
    from safetensors.torch import load_file
    with safe_open(path, framework="pt") as f:
        meta = f.metadata() or {}
    if meta.get("algo", "td3") != "td3":
        raise ValueError("%s is a '%s' checkpoint, not a td3 one" % (path, meta["algo"]))
    sd = load_file(path)
    pol = {k[len("policy."):]: v for k, v in sd.items() if k.startswith("policy.")}
    arch = tuple(int(n) for n in meta["net_arch"].split(",")) if "net_arch" in meta else (64, 64)
    model = Td3Policy(pol["actor.0.weight"].shape[1], pol["actor.%d.bias" % (2 * len(arch))].shape[0], arch, meta.get("activation", "tanh"))
    model.load_state_dict(pol)
    return model, {k[len("vecnormalize."):]: v for k, v in sd.items() if k.startswith("vecnormalize.")}
