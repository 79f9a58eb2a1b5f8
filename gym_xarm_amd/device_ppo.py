"""Device-resident PPO update: stable-baselines3's `PPO.train()` on a stored rollout - GAE(lambda), `n_epochs` passes over shuffled
minibatches, per-minibatch advantage normalisation, the clipped surrogate, the backward of both towers, `clip_grad_norm_` and
`Adam.step` - as one stream-ordered call of 4 + 3 S HIP launches, S = n_epochs x minibatches (csrc/xarm_k_ppo.hip).

A torch PPO update is S times the launch chain of an A2C update (forward of both towers under autograd, backward, clip, optimiser);
`DevicePPO` keeps the rollout in the buffers `DeviceA2C` uses and updates the module's own parameter tensors in place, so a
`DevicePolicy` on the same module (or the module itself) sees the new weights in its next call.  The checker is the torch PPO block of
train.py - ppo_prepare, ppo_minibatch_loss and optimizer_step, which train() itself runs through ppo_update without device_update:
tests/ppo_host.py calls them on float64 and float32 copies of the model (tests/test_ppo_host.py, tests/test_ppo_gpu.py)."""
import ctypes as C

import torch

from . import _native
from .device_a2c import acw_weights, module_params, policy_weights
from .device_policy import is_tile64, tower_params, tower_shape, wide_supported
from .train import rollout_buffers, store_rollout


def _check_adam(opt):
    for g in opt.param_groups:
        if g.get("amsgrad", False) or g.get("weight_decay", 0) != 0 or g.get("maximize", False):
            raise ValueError("the device update is Adam without amsgrad, weight decay or maximize")


def load_adam(exp_avg, exp_avg_sq, step, opt, params):
    """copy the state of a torch.optim.Adam built on `params` into the 13 + 13 state tensors and the step counter (zeros for a
    parameter the optimiser has not stepped yet)"""
    _check_adam(opt)
    steps = set()
    with torch.no_grad():
        for m, v, p in zip(exp_avg, exp_avg_sq, params):
            st = opt.state.get(p, {})
            if "exp_avg" in st:
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
                steps.add(int(st["step"]))
            else:
                m.zero_()
                v.zero_()
                steps.add(0)
        if len(steps) != 1:
            raise ValueError("the device update keeps one step count for all parameters; the optimiser holds %s" % sorted(steps))
        step.fill_(steps.pop())


def export_adam(exp_avg, exp_avg_sq, step, opt, params):
    """the other direction: the optimiser continues from the state tensors and the step counter (reads `step` back)"""
    _check_adam(opt)
    t = float(int(step.item()))
    with torch.no_grad():
        for m, v, p in zip(exp_avg, exp_avg_sq, params):
            st = opt.state[p]
            if "exp_avg" in st:
                st["exp_avg"].copy_(m)
                st["exp_avg_sq"].copy_(v)
                st["step"].fill_(t)
            else:
                st["step"] = torch.tensor(t, dtype=torch.float32)
                st["exp_avg"] = m.detach().clone()
                st["exp_avg_sq"] = v.detach().clone()


class DevicePPO:
    """One PPO update per `update()` call on the model's GPU.

    model: a train.ActorCritic whose parameters are contiguous float32 CUDA tensors; they are read and written in place.
    `buffers` and `store(k, ...)` are DeviceA2C's.  `exp_avg`, `exp_avg_sq` (13 tensors each) and `step` (int64 [1]) are Adam's state,
    `perm` (int32 [n_epochs, N]) the minibatch order: all device tensors.  shuffle: what refills `perm` in front of an update - "torch"
    (torch.randperm per epoch) or "device" (xarm_perm_fill, csrc/xarm_k_rollout.hip, DESIGN.md 27: capturable; `perm_calls` int64 [1] counts
    its draws).  `stats` [S, 8]: one row per optimiser step of the last update,
    policy_loss, value_loss, entropy, grad_norm, n_use, approx_kl, clip_fraction, stopped.  batch_size None: ceil(N / 4).

    clip_range_vf (None: off): stable-baselines3's value clipping against the values at call start.  target_kl (None: off): SB3's early
    stop, taken on the device - the first optimiser step whose approx_kl exceeds 1.5 target_kl, and every step after it, is not applied
    (no parameter, no Adam state, no advance of `step`), with no host read, so the call stays capturable.  `stats[:, 7]` is 0 for an
    applied step and 1 for one that was not; the tripping row keeps its sums with grad_norm 0, later rows are zero.  Both live in
    `hyper`; `set_hyper(lr=..., clip_range=..., clip_range_vf=...)` rewrites entries of it between updates (train()'s schedules).  A
    captured graph holds the hyper-parameters of its capture: schedules do not reach into it.

    `backend`: "tile64" - the fused 64-row tile of DESIGN.md 22, 4 + 3 S launches, for a 64-64 tanh model - or "wide" - the per-layer MFMA
    GEMM chain of DESIGN.md 25 (csrc/xarm_k_ppow.hip) for equal widths of 64, 128, 192 or 256 units in two or three layers, tanh or ReLU,
    the reference's [256, 256, 256] among them.  wide None: "tile64" for a 64-64 tanh model and "wide" for every other supported shape;
    wide=True forces "wide".  `exp_avg` / `exp_avg_sq` hold one tensor per parameter in the order of `params()`: pi's tensors, vf's,
    log_std.  `launches`: the kernels of one update - 4 + 3 S, or on the wide backend c (L + 1) + 2 + S (2 L + 6) with L hidden layers and
    c = M + ceil(E / B) call-start forward chunks."""

    def __init__(self, model, num_envs, n_steps=16, n_epochs=4, batch_size=None, gamma=0.99, gae_lambda=0.95, clip_range=0.2, lr=3e-4,
                 betas=(0.9, 0.999), eps=1e-5, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5, normalize_advantage=True, seed=0, wide=None,
                 clip_range_vf=None, target_kl=None, shuffle="torch"):
        if shuffle not in ("torch", "device"):
            raise ValueError("DevicePPO: shuffle must be 'torch' or 'device', not %r" % (shuffle,))
        self.shuffle_mode, self.seed = shuffle, int(seed)
        self.model, self.num_envs, self.n_steps, self.n_epochs = model, int(num_envs), int(n_steps), int(n_epochs)
        N = self.num_envs * self.n_steps
        self.batch_size = int(batch_size) if batch_size is not None else max(1, -(-N // 4))
        self.hyper = dict(gamma=gamma, gae_lambda=gae_lambda, clip_range=clip_range, lr=lr, beta1=betas[0], beta2=betas[1], eps=eps, vf_coef=vf_coef,
                          ent_coef=ent_coef, max_grad_norm=max_grad_norm, clip_range_vf=clip_range_vf, target_kl=target_kl)
        self.normalize_advantage = bool(normalize_advantage)
        self.obs_width = int(model.pi[0].in_features)
        self.act_dim = int(model.pi[-1].out_features)
        self.widths, self.activation = tower_shape(model)
        if wide is False and not is_tile64(model):
            raise ValueError("DevicePPO: the fused tile (wide=False) updates 64-64 tanh towers (XARM_POLICY_HIDDEN), not %s %s"
                             % (list(self.widths), self.activation))
        self.backend = "tile64" if is_tile64(model) and not wide else "wide"
        if self.backend == "wide" and not wide_supported(model):
            raise ValueError("DevicePPO updates 64-64 tanh towers (the fused tile) and equal-width towers of 2 or 3 hidden layers of 64, 128, 192 or 256 units, tanh or relu, not "
                             "%s %s; train.ppo_update is the torch implementation for every other shape" % (list(self.widths), self.activation))
        self.device = model.log_std.device
        if self.device.type != "cuda":
            raise ValueError("DevicePPO runs the update with HIP kernels on the model's GPU: the model is on '%s'.  There is no host "
                             "path; the torch PPO block of train.py (autograd, clip_grad_norm_, Adam) is the host implementation." % self.device)
        self._L = _native.load()
        T, E, D, A, dev = self.n_steps, self.num_envs, self.obs_width, self.act_dim, self.device
        nbytes = C.c_int64(0)
        self.minibatches = -(-N // min(self.batch_size, N)) if N > 0 else 0
        self.num_steps = self.n_epochs * self.minibatches
        if self.backend == "wide":
            L = len(self.widths)
            self._layout = _native.XarmPPOWLayout(E, T, D, A, self.widths[0], L, _native.SACW_ACTIVATIONS[self.activation], self.n_epochs, self.batch_size)
            _native.check(self._L, None, self._L.xarm_ppow_workspace_bytes(C.byref(self._layout), C.byref(nbytes)), "xarm_ppow_workspace_bytes")
            chunks = self.minibatches + (-(-E // min(self.batch_size, N)) if N > 0 else 0)
            self.launches = chunks * (L + 1) + 2 + self.num_steps * (2 * L + 6)
        else:
            self._layout = _native.XarmPPOLayout(E, T, D, A, _native.POLICY_HIDDEN, self.n_epochs, self.batch_size)
            _native.check(self._L, None, self._L.xarm_ppo_workspace_bytes(C.byref(self._layout), C.byref(nbytes)), "xarm_ppo_workspace_bytes")
            self.launches = 4 + 3 * self.num_steps
        self.buffers = rollout_buffers(T, E, D, A, dev, nbytes.value)
        self.exp_avg = [torch.zeros_like(p) for p in self.params()]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params()]
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.perm = torch.arange(N, dtype=torch.int32, device=dev).repeat(self.n_epochs, 1).contiguous()
        self.stats = torch.zeros(max(self.num_steps, 1), 8, device=dev)
        self.num_params = sum(p.numel() for p in self.params())
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(int(seed))
        self.perm_calls = torch.zeros(1, dtype=torch.int64, device=dev) if shuffle == "device" else None    # shuffles drawn so far

    def params(self):
        """the trained tensors in the flat order of out_grad: pi's W1, b1, ..., vf's, log_std (the 13 of xarm_policy_weights on "tile64")"""
        if self.backend == "wide":
            pi, vf = tower_params(self.model)
            return pi + vf + (self.model.log_std,)
        return module_params(self.model)

    def _wide_weights(self, tensors):
        return acw_weights(tensors, self.device, "DevicePPO")

    def set_hyper(self, **kw):
        """rewrite entries of `hyper` (lr, clip_range, clip_range_vf, ...): the next update reads them"""
        for k, v in kw.items():
            if k not in self.hyper:
                raise KeyError("DevicePPO has no hyper-parameter %r (it has %s)" % (k, ", ".join(sorted(self.hyper))))
            self.hyper[k] = v

    def store(self, k, obs, action, reward, done, resetting=None):
        """slot k of the rollout (train.store_rollout)"""
        store_rollout(self.buffers, k, obs, action, reward, done, resetting)

    def shuffle(self):
        """a fresh permutation per epoch, in place.  shuffle="torch": torch.randperm from the object's own seeded device generator
        (allocates: not for a capture).  shuffle="device": xarm_perm_fill keyed by (seed, `perm_calls`) on the current stream - two launches,
        no allocation, no host read; the fill advances `perm_calls` on the device, so a captured call draws a fresh shuffle per replay."""
        N = self.num_envs * self.n_steps
        if self.shuffle_mode == "device":
            rc = self._L.xarm_perm_fill(C.c_void_p(self.perm.data_ptr()), self.n_epochs, N, self.seed, C.c_void_p(self.perm_calls.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
            _native.check(self._L, None, rc, "xarm_perm_fill")
            return
        for ep in range(self.n_epochs):
            self.perm[ep].copy_(torch.randperm(N, generator=self._gen, device=self.device))

    def _call(self, weights, exp_avg, exp_avg_sq, step, last_obs, hyper, old_logp, out_adv, out_returns, out_grad, out_stats):
        E, D, T = self.num_envs, self.obs_width, self.n_steps
        assert last_obs.dtype == torch.float32 and last_obs.is_contiguous() and tuple(last_obs.shape) == (E, D) and last_obs.device == self.device, \
            "last_obs must be a contiguous float32 [num_envs, D] tensor on the model's device"
        for t, shape in ((old_logp, (T, E)), (out_adv, (T, E)), (out_returns, (T, E)), (out_grad, (self.num_params,))):
            assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape and t.device == self.device), \
                "old_logp / out_adv / out_returns [n_steps, num_envs] and out_grad [num_params]: contiguous float32 on the model's device"
        b = self.buffers
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        params = _native.XarmPPOParams(*([float(hyper[k]) for k in _native.PPO_HYPER] + [int(self.normalize_advantage)]))
        vclip, kl = hyper.get("clip_range_vf"), hyper.get("target_kl")
        options = None if vclip is None and kl is None else C.byref(_native.XarmPPOOptions(float(vclip or 0.0), float(kl or 0.0)))
        args = (p(step), p(b["obs"]), p(b["action"]), p(b["reward"]), p(b["done"]), p(b["use"]), p(last_obs), p(old_logp), p(self.perm), p(b["workspace"]),
                p(out_adv), p(out_returns), p(out_grad), p(out_stats), options, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if self.backend == "wide":
            ws = [self._wide_weights(ts) for ts in (weights, exp_avg, exp_avg_sq)]        # held until the call has returned
            rc = self._L.xarm_ppow_update_opt(C.byref(self._layout), C.byref(params), *[C.byref(x) for x in ws], *args)
            _native.check(self._L, None, rc, "xarm_ppow_update")
            return
        ws = [policy_weights(ts, self.device, "DevicePPO") for ts in (weights, exp_avg, exp_avg_sq)]
        rc = self._L.xarm_ppo_update_opt(C.byref(self._layout), C.byref(params), *[C.byref(x) for x in ws], *args)
        _native.check(self._L, None, rc, "xarm_ppo_update")

    def update(self, last_obs, shuffle=True, old_logp=None, out_adv=None, out_returns=None, out_grad=None):
        """one update from the stored rollout and the observation after its last step; the module's parameters, Adam's state and `step`
        change in place, `stats` is rewritten.  shuffle: refill `perm` first.  With shuffle=False, or on a DevicePPO(shuffle="device"),
        nothing is allocated and nothing is read back, so the call can be captured in a torch.cuda.graph - with the device shuffle inside
        it; a captured user of the torch shuffle calls shuffle() between replays.  old_logp [T, E]:
        used in place of the log-probabilities at call start.  out_adv / out_returns [T, E], out_grad [num_params] (debug): the
        advantages before normalisation, the returns and step 0's gradient before the clip."""
        if shuffle:
            self.shuffle()
        self._call(self.params(), self.exp_avg, self.exp_avg_sq, self.step, last_obs, self.hyper, old_logp, out_adv, out_returns, out_grad, self.stats)
        return self.stats

    def grad(self, last_obs, old_logp=None):
        """(step 0's flat gradient before the clip [num_params], adv [T, E], returns [T, E], stats [S, 8]) of the stored rollout and the
        present `perm`, computed by the same call on scratch copies of the weights and of Adam's state with lr = 0: the module is not
        touched (debug; allocates)"""
        w, m, v = [p.detach().clone() for p in self.params()], [s.clone() for s in self.exp_avg], [s.clone() for s in self.exp_avg_sq]
        dev, T, E = self.device, self.n_steps, self.num_envs
        g, a, r, st = torch.empty(self.num_params, device=dev), torch.empty(T, E, device=dev), torch.empty(T, E, device=dev), torch.zeros_like(self.stats)
        self._call(w, m, v, self.step.clone(), last_obs, dict(self.hyper, lr=0.0), old_logp, a, r, g, st)
        return g, a, r, st

    def steps_applied(self):
        """optimiser steps the last update applied, from `stats[:, 7]` (reads back: not for a capture)"""
        return int((self.stats[:self.num_steps, 7] == 0).sum().item())

    def load_optimizer(self, opt):
        """continue from a torch.optim.Adam built on the same module"""
        load_adam(self.exp_avg, self.exp_avg_sq, self.step, opt, self.params())

    def export_optimizer(self, opt):
        """let a torch.optim.Adam built on the same module continue from this updater's state"""
        export_adam(self.exp_avg, self.exp_avg_sq, self.step, opt, self.params())
