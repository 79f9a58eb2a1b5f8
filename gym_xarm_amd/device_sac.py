"""Device-resident SAC: one gradient step of stable-baselines3's `SAC.train()` - the squashed-Gaussian actor on obs and next_obs, the
entropy coefficient's step, the soft target, the step of both critics, the actor's step through the stepped critics and the Polyak
step of the targets - as one stream-ordered call of six HIP launches, and the actor's rollout / deployment call as one launch
(csrc/xarm_k_sac.hip).

The torch block of gym_xarm_amd/sac.py runs three autograd passes and three `Adam.step`s per SAC step, a few hundred small launches;
`DeviceSAC` updates the `SacPolicy`'s own parameter tensors in place, so the module (and a checkpoint written from it) always holds the
current weights.  The torch block stays as it is and is the checker (tests/test_sac_host.py, tests/test_sac_gpu.py).

A model of another equal-width shape - two or three hidden layers of 64, 128, 192 or 256 units, tanh or ReLU, the reference's
[256, 256, 256] among them - takes the "wide" backend (csrc/xarm_k_sacw.hip): the same step as a chain of 6 n_hidden + 11
launches whose dense work runs on f32 MFMA GEMMs (tests/test_sacw_host.py, tests/test_sacw_gpu.py)."""
import ctypes as C

import torch

from . import _native
from .device_ppo import export_adam, load_adam
from .replay import DeviceReplayBuffer


def tower_params(seq):
    """W1, b1, ..., W_out, b_out of a tower: its nn.Linear layers in order (six tensors for a 64-64 tower)"""
    return tuple(t for m in seq if isinstance(m, torch.nn.Linear) for t in (m.weight, m.bias))


def module_params(model):
    """the tensors of a sac.SacPolicy in the order of include/xarm_hip.h xarm_sac_weights / xarm_sacw_weights: actor, q1, q2, q1_target,
    q2_target, log_alpha - 2 (n_hidden + 1) per tower, so 31 for two hidden layers and 41 for three"""
    return tower_params(model.actor) + tower_params(model.q1) + tower_params(model.q2) + tower_params(model.q1_target) + \
        tower_params(model.q2_target) + (model.log_alpha,)


def trained(tensors):
    """the trained of module_params' tensors, in the flat order of the gradient: actor's, q1's, q2's, log_alpha (19 of 31, 25 of 41)"""
    n = 3 * ((len(tensors) - 1) // 5)
    return tuple(tensors[:n]) + (tensors[-1],)


def sacw_weights(tensors, device, who="DeviceSAC"):
    """module_params' tensors (or the trained ones: the target fields stay NULL) as an xarm_sacw_weights of device pointers"""
    full = (len(tensors) - 1) % 5 == 0 and (len(tensors) - 1) // 5 in (6, 8)
    tp = (len(tensors) - 1) // (5 if full else 3)
    w = _native.XarmSACWWeights()
    for i, t in enumerate(tensors):
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
            raise ValueError("%s needs contiguous float32 tensors on %s (tensor %d)" % (who, device, i))
        if i == len(tensors) - 1:
            w.log_alpha = t.data_ptr()
        else:
            getattr(w, _native.SAC_TOWERS[i // tp])[i % tp] = t.data_ptr()
    return w


def model_shape(model):
    """(hidden widths of every tower, activation) of a sac.SacPolicy"""
    widths = [tuple(int(m.out_features) for m in t if isinstance(m, torch.nn.Linear))[:-1] for t in (model.actor, model.q1, model.q2, model.q1_target, model.q2_target)]
    kinds = {type(m) for t in (model.actor, model.q1, model.q2, model.q1_target, model.q2_target) for m in t if not isinstance(m, torch.nn.Linear)}
    act = "tanh" if kinds == {torch.nn.Tanh} else ("relu" if kinds == {torch.nn.ReLU} else None)
    return widths, act


def sac_weights(tensors, device, who="DeviceSAC"):
    """31 tensors (or 19: the trained ones, the target fields stay NULL) as an xarm_sac_weights of device pointers"""
    if len(tensors) == 19:
        tensors = tuple(tensors[:18]) + (None,) * 12 + (tensors[18],)
    w = _native.XarmSACWeights()
    for i, t in enumerate(tensors):
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
            raise ValueError("%s needs contiguous float32 tensors on %s (tensor %d)" % (who, device, i))
        if i == 30:
            w.log_alpha = t.data_ptr()
        else:
            getattr(w, _native.SAC_TOWERS[i // 6])[i % 6] = t.data_ptr()
    return w


class DeviceSAC:
    """One SAC step per `update()` call on the model's GPU, and the actor's `act_into` / `predict`.

    model: a sac.SacPolicy whose parameters are contiguous float32 CUDA tensors; they are read and written in place.
    `exp_avg`, `exp_avg_sq` (the trained tensors each: actor, q1, q2, log_alpha) and `step` (int64 [1]) are the state of the torch block's
    three Adams, which step together; `stats` [8] = critic_loss, actor_loss, alpha_loss, alpha, mean logp_pi, mean min-Q, n_use, 0 of the
    last step; `calls` (int64 [1]) counts the stochastic `act_into` calls.  All are device tensors.

    `backend`: "tile64" - the fused 64-row tile of DESIGN.md 23, six launches, for a 64-64 tanh model - or "wide" - the per-layer MFMA
    GEMM chain of DESIGN.md 24 for equal widths of 64, 128, 192 or 256 units, two or three hidden layers, tanh or ReLU.  wide=None picks
    "tile64" for a 64-64 tanh model and "wide" for every other supported shape; wide=True forces "wide".  act_rows: the most rows an `act_into` call will carry on the wide backend
    (default batch_size): its layer-by-layer forward keeps activations in ONE workspace, sized here (`reserve_act` resizes it).  `launches`: the kernels of one
    step, a function of the backend and the depth alone (6; 6 n_hidden + 11)."""

    launches = 6

    def __init__(self, model, batch_size, gamma=0.95, lr=1e-3, tau=0.005, ent_coef="auto", target_entropy=None, betas=(0.9, 0.999), eps=1e-8, seed=0,
                 row_offset=0, wide=None, act_rows=None):
        self.model, self.batch_size, self.seed, self.row_offset = model, int(batch_size), int(seed), int(row_offset)
        self.obs_width, self.act_dim = int(model.actor[0].in_features), int(model.actor[len(model.actor) - 1].out_features) // 2
        widths, act = model_shape(model)
        tile64 = all(w == (_native.POLICY_HIDDEN,) * 2 for w in widths) and act == "tanh"
        if wide is False and not tile64:
            raise ValueError("DeviceSAC(wide=False) is the 64-64 tanh tile (XARM_POLICY_HIDDEN); this model's towers are %s %s" % (widths[0], act))
        self.backend = "tile64" if tile64 and not wide else "wide"
        if self.backend == "wide":
            arch = widths[0]
            why = None
            if any(w != arch for w in widths) or len(set(arch)) != 1:
                why = "every hidden layer of every tower must have the same width (towers: %s)" % (widths,)
            elif len(arch) not in (2, 3):
                why = "two or three hidden layers (the model has %d)" % len(arch)
            elif arch[0] not in _native.SACW_WIDTHS:
                why = "a hidden width of 64, 128, 192 or 256 (the model's is %d)" % arch[0]
            elif act is None:
                why = "tanh or ReLU between the layers"
            if why is not None:
                raise ValueError("DeviceSAC's kernels need %s.  The torch block (gym_xarm_amd/sac.py sac_step with make_optimizers) runs "
                                 "every shape." % why)
            self.hidden, self.n_hidden, self.activation = int(arch[0]), len(arch), act
            self.launches = 6 * self.n_hidden + 11
        self.auto = ent_coef == "auto"
        self.hyper = dict(gamma=gamma, lr=lr, tau=tau, ent_coef=0.0 if self.auto else float(ent_coef),
                          target_entropy=-float(self.act_dim) if target_entropy is None else float(target_entropy), beta1=betas[0], beta2=betas[1], eps=eps)
        self.device = model.log_alpha.device
        if self.device.type != "cuda":
            raise ValueError("DeviceSAC runs the SAC step with HIP kernels on the model's GPU: the model is on '%s'.  There is no host path; "
                             "the torch block of train_sac (gym_xarm_amd/sac.py sac_step: autograd and three Adams) is the host "
                             "implementation." % self.device)
        self._L = _native.load()
        B, D, A, dev = self.batch_size, self.obs_width, self.act_dim, self.device
        nbytes = C.c_int64(0)
        if self.backend == "wide":
            self._layout = self._wide_layout(B)
            _native.check(self._L, None, self._L.xarm_sacw_workspace_bytes(C.byref(self._layout), C.byref(nbytes)), "xarm_sacw_workspace_bytes")
            self._act_work = None
        else:
            self._layout = _native.XarmSACLayout(B, D, A, _native.POLICY_HIDDEN, self.row_offset)
            _native.check(self._L, None, self._L.xarm_sac_workspace_bytes(C.byref(self._layout), C.byref(nbytes)), "xarm_sac_workspace_bytes")
        self.buffers = {"obs": torch.zeros(B, D, device=dev), "next_obs": torch.zeros(B, D, device=dev), "done": torch.zeros(B, device=dev),
                        "use": torch.ones(B, device=dev), "workspace": torch.zeros(max(nbytes.value, 16) // 4, dtype=torch.float32, device=dev)}
        self.exp_avg = [torch.zeros_like(p) for p in trained(self.params())]
        self.exp_avg_sq = [torch.zeros_like(p) for p in trained(self.params())]
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.calls = torch.zeros(1, dtype=torch.int64, device=dev)
        self.stats = torch.zeros(8, device=dev)
        self.num_params = sum(p.numel() for p in trained(self.params()))
        if self.backend == "wide":
            self.reserve_act(act_rows if act_rows is not None else B)

    def params(self):
        return module_params(self.model)

    def reserve_act(self, rows):
        """wide backend: make the act call's workspace hold `rows` rows (one tensor, kept; a call with more rows than it holds grows it,
        which allocates - reserve before a graph capture)"""
        n = self.n_hidden * rows * self.hidden + 2 * self.act_dim * rows + 16
        if self._act_work is None or self._act_work.numel() < n:
            self._act_work = torch.zeros(n, dtype=torch.float32, device=self.device)

    def _wide_layout(self, rows):
        return _native.XarmSACWLayout(rows, self.obs_width, self.act_dim, self.hidden, self.n_hidden, _native.SACW_ACTIVATIONS[self.activation],
                                      self.row_offset)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _params(self, hyper, deterministic=False):
        return _native.XarmSACParams(*([self.seed] + [float(hyper[k]) for k in _native.SAC_HYPER] + [int(self.auto), int(deterministic)]))

    def _check(self, t, shape, what):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape and t.device == self.device, \
            "%s must be a contiguous float32 %s tensor on the model's device" % (what, list(shape))
        return t

    def _call(self, weights, exp_avg, exp_avg_sq, step, b, hyper, noise_pi=None, noise_next=None, out_grad=None, out_dqda=None, out_target=None,
              out_stats=None, out_q=None):
        B, D, A = self.batch_size, self.obs_width, self.act_dim
        self._check(b["obs"], (B, D), "obs"); self._check(b["next_obs"], (B, D), "next_obs"); self._check(b["action"], (B, A), "action")
        self._check(b["reward"], (B,), "reward"); self._check(b["done"], (B,), "done")
        for t, shape, k in ((b.get("use"), (B,), "use"), (noise_pi, (B, A), "noise_pi"), (noise_next, (B, A), "noise_next"),
                            (out_grad, (self.num_params,), "out_grad"), (out_dqda, (2, B, A), "out_dqda"), (out_target, (B,), "out_target"),
                            (out_q, (2, B), "out_q")):
            if t is not None:
                self._check(t, shape, k)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        if self.backend == "wide":
            W = lambda ts: C.byref(sacw_weights(ts, self.device))
            rc = self._L.xarm_sacw_update(C.byref(self._layout), C.byref(self._params(hyper)), W(weights), W(exp_avg), W(exp_avg_sq), p(step), p(b["obs"]),
                                          p(b["next_obs"]), p(b["action"]), p(b["reward"]), p(b["done"]), p(b.get("use")), p(noise_pi), p(noise_next),
                                          p(self.buffers["workspace"]), p(out_grad), p(out_dqda), p(out_target), p(out_stats), p(out_q), self._stream())
            _native.check(self._L, None, rc, "xarm_sacw_update")
            return
        assert out_q is None, "out_q is the wide backend's output"
        W = lambda ts: C.byref(sac_weights(ts, self.device))
        rc = self._L.xarm_sac_update(C.byref(self._layout), C.byref(self._params(hyper)), W(weights), W(exp_avg), W(exp_avg_sq), p(step), p(b["obs"]),
                                     p(b["next_obs"]), p(b["action"]), p(b["reward"]), p(b["done"]), p(b.get("use")), p(noise_pi), p(noise_next),
                                     p(self.buffers["workspace"]), p(out_grad), p(out_dqda), p(out_target), p(out_stats), self._stream())
        _native.check(self._L, None, rc, "xarm_sac_update")

    def update(self, batch, noise_pi=None, noise_next=None):
        """one SAC step on batch = {"obs", "next_obs" [B, D] (flat, normalised), "action" [B, A], "reward", "done" [B], optional "use" [B]}:
        contiguous float32 tensors on the model's device.  The module's parameters and targets, Adam's state and `step` change in place,
        `stats` is rewritten.  noise_pi / noise_next [B, A]: the step's z in place of the Philox draw.  No allocation, no host read;
        capturable."""
        self._call(self.params(), self.exp_avg, self.exp_avg_sq, self.step, batch, self.hyper, noise_pi, noise_next, out_stats=self.stats)
        return self.stats

    def update_from(self, buffer, normalize=None, sample=None):
        """sample `buffer` (a DeviceHerReplayBuffer) and step: `buffer.sample_into` with its relabelled rewards, the two observation
        triples concatenated and normalised by `normalize` (a DeviceVecNormalize: one xarm_norm_obs launch each with update = 0; None:
        concatenated as they are), `ok` as use, then `update`.  sample: `buffer.alloc_out(batch_size)` tensors to reuse (allocated at
        the first call otherwise).  After the first call no allocation and no host read; capturable.
        A DeviceReplayBuffer (gym_xarm_amd/replay.py) takes the short way: `_update_from_uniform`."""
        if isinstance(buffer, DeviceReplayBuffer):
            return self._update_from_uniform(buffer, normalize, sample)
        if sample is None:
            if getattr(self, "_sample", None) is None:
                self._sample = buffer.alloc_out(self.batch_size)
            sample = self._sample
        s, b = buffer.sample_into(sample), self.buffers
        first, second = (s["observation"], s["achieved_goal"], s["desired_goal"]), (s["next_observation"], s["next_achieved_goal"], s["desired_goal"])
        if normalize is not None:
            if int(normalize.dim) != self.obs_width:
                raise ValueError("DeviceSAC: the normaliser's statistics do not belong to this model's observation")
            normalize.normalize_rows(b["obs"], *first)
            normalize.normalize_rows(b["next_obs"], *second)
        else:
            torch.cat(first, dim=1, out=b["obs"])
            torch.cat(second, dim=1, out=b["next_obs"])
        b["done"].copy_(s["done"])
        b["use"].copy_(s["ok"])
        return self.update({"obs": b["obs"], "next_obs": b["next_obs"], "action": s["action"], "reward": s["reward"], "done": b["done"], "use": b["use"]})

    def _update_from_uniform(self, buffer, normalize=None, sample=None):
        """update_from on a DeviceReplayBuffer: its sample kernel writes the batch where `update` reads it - `buffers`' obs, next_obs (normalised
        in the kernel by `normalize`'s statistics), done and use, and the action / reward tensors of `sample` (buffer.alloc_out's; two tensors
        of this updater's, allocated at the first call, otherwise) - and `update` runs behind it: no torch op in between."""
        if buffer.dim != self.obs_width or buffer.act_dim != self.act_dim:
            raise ValueError("%s: the buffer's rows (observation %d, action %d) do not belong to this model (%d, %d)"
                             % (type(self).__name__, buffer.dim, buffer.act_dim, self.obs_width, self.act_dim))
        if sample is None:
            if getattr(self, "_uniform_sample", None) is None:
                self._uniform_sample = {"action": torch.empty(self.batch_size, self.act_dim, device=self.device),
                                        "reward": torch.empty(self.batch_size, device=self.device)}
            sample = self._uniform_sample
        b = self.buffers
        batch = {"obs": b["obs"], "next_obs": b["next_obs"], "action": sample["action"], "reward": sample["reward"], "done": b["done"], "use": b["use"]}
        buffer.sample_into(batch, normalize)
        return self.update(batch)

    def act_into(self, out, obs, deterministic=False):
        """One launch (n_hidden + 2 on the wide backend; plus the counter tick of a stochastic call): out["action"] [E, A] = tanh(mean + exp(log_std) z) (tanh(mean) when
        deterministic) and, where the dict has it, out["logp"] [E], for the normalised flat observation obs [E, D].  Noise: Philox keyed
        by (seed, row_offset + row, calls, column block) as DevicePolicy's.  No allocation, no host read; capturable."""
        E, A = int(obs.shape[0]), self.act_dim
        self._check(obs, (E, self.obs_width), "obs"); self._check(out["action"], (E, A), "out['action']")
        if "logp" in out:
            self._check(out["logp"], (E,), "out['logp']")
        if self.backend == "wide":
            self.reserve_act(E)
            rc = self._L.xarm_sacw_act(C.byref(self._wide_layout(E)), C.byref(self._params(self.hyper, deterministic)),
                                       C.byref(sacw_weights(self.params(), self.device)), C.c_void_p(self.calls.data_ptr()), C.c_void_p(obs.data_ptr()),
                                       C.c_void_p(self._act_work.data_ptr()), C.c_void_p(out["action"].data_ptr()),
                                       C.c_void_p(out["logp"].data_ptr()) if "logp" in out else None, self._stream())
            _native.check(self._L, None, rc, "xarm_sacw_act")
            return out
        layout = _native.XarmSACLayout(E, self.obs_width, A, _native.POLICY_HIDDEN, self.row_offset)
        rc = self._L.xarm_sac_act(C.byref(layout), C.byref(self._params(self.hyper, deterministic)), C.byref(sac_weights(self.params(), self.device)),
                                  C.c_void_p(self.calls.data_ptr()), C.c_void_p(obs.data_ptr()), C.c_void_p(out["action"].data_ptr()),
                                  C.c_void_p(out["logp"].data_ptr()) if "logp" in out else None, self._stream())
        _native.check(self._L, None, rc, "xarm_sac_act")
        return out

    def predict(self, obs, deterministic=True):
        """the deployment call: the action [E, A] for the normalised flat observation"""
        return self.act_into({"action": torch.empty(int(obs.shape[0]), self.act_dim, device=self.device)}, obs, deterministic)["action"]

    def grad(self, batch, noise_pi=None, noise_next=None, lr=0.0):
        """{"grad" [num_params] (actor's 6 tensors, q1's, q2's, log_alpha), "actor", "critic", "log_alpha" (views of it), "dqda" [2, B, A],
        "y" [B], "stats" [8], and on the wide backend "q" [2, B]: q1, q2 at obs | action} of one step on scratch copies of the weights and of Adam's state with lr = 0: the module is not touched
        (debug; allocates).  With lr = 0 the critics at the actor step are the critics at call start; with the updater's own lr the
        actor's gradient and dq/da are what `update` computes - through the stepped critics."""
        w = [p.detach().clone() for p in self.params()]
        m, v = [s.clone() for s in self.exp_avg], [s.clone() for s in self.exp_avg_sq]
        dev, B, A = self.device, self.batch_size, self.act_dim
        g, dq, y, st = torch.empty(self.num_params, device=dev), torch.empty(2, B, A, device=dev), torch.empty(B, device=dev), torch.zeros(8, device=dev)
        q = torch.empty(2, B, device=dev) if self.backend == "wide" else None
        self._call(w, m, v, self.step.clone(), batch, dict(self.hyper, lr=float(lr)), noise_pi, noise_next, g, dq, y, st, q)
        tp = (len(self.params()) - 1) // 5
        na = sum(p.numel() for p in self.params()[:tp])
        out = {"grad": g, "actor": g[:na], "critic": g[na:-1], "log_alpha": g[-1:], "dqda": dq, "y": y, "stats": st}
        if q is not None:
            out["q"] = q
        return out

    def _groups(self, opts):
        ps = trained(self.params())
        tp = (len(ps) - 1) // 3
        return (("actor", slice(0, tp)), ("critic", slice(tp, 3 * tp)), ("alpha", slice(3 * tp, 3 * tp + 1))), ps

    def load_optimizer(self, opts):
        """continue from the torch block's Adams, opts = {"actor", "critic", "alpha"} (sac.make_optimizers; "alpha" None with a fixed
        ent_coef).  They must have taken the same number of steps."""
        groups, ps = self._groups(opts)
        steps = []
        for k, sl in groups:
            if opts.get(k) is None:
                continue
            st = torch.zeros(1, dtype=torch.int64, device=self.device)
            load_adam(self.exp_avg[sl], self.exp_avg_sq[sl], st, opts[k], ps[sl])
            steps.append(int(st.item()))
        if len(set(steps)) != 1:
            raise ValueError("the device update keeps one step count for the three optimisers; they hold %s" % steps)
        self.step.fill_(steps[0])

    def export_optimizer(self, opts):
        """let the torch block's Adams, built on the same module, continue from this updater's state (reads `step` back)"""
        groups, ps = self._groups(opts)
        for k, sl in groups:
            if opts.get(k) is not None:
                export_adam(self.exp_avg[sl], self.exp_avg_sq[sl], self.step, opts[k], ps[sl])
