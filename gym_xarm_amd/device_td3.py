"""Device-resident TD3: one gradient step of stable-baselines3's `TD3.train()` - target policy smoothing, the clipped double-Q target,
the step of both critics and, on every policy_delay-th call, the actor's step through dq1/da and the Polyak step of the three targets -
as one stream-ordered call of 7 n_hidden + 14 HIP launches, and the actor's rollout / deployment call (csrc/xarm_k_td3.hip).

Whether a call steps the actor is decided on the device from the step count, so a captured `update` replays correctly.  `DeviceTD3`
updates the `Td3Policy`'s own parameter tensors in place; the torch block of gym_xarm_amd/td3.py stays as it is and is the checker
(tests/test_td3_host.py, tests/test_td3_gpu.py).  Shapes: equal widths of 64, 128, 192 or 256 units, two or three hidden layers, tanh
or ReLU - the dense work runs on the wide SAC's f32 MFMA GEMM kernels."""
import ctypes as C

import torch

from . import _native
from .device_ppo import export_adam, load_adam
from .replay import DeviceReplayBuffer
from .device_sac import tower_params


def module_params(model):
    """the tensors of a td3.Td3Policy in the order of include/xarm_hip.h xarm_td3_weights: actor, q1, q2, actor_target, q1_target,
    q2_target - 2 (n_hidden + 1) per tower"""
    return tuple(t for name in _native.TD3_TOWERS for t in tower_params(getattr(model, name)))


def trained(tensors):
    """the trained of module_params' tensors, in the flat order of the gradient: actor's, q1's, q2's (the first half)"""
    return tuple(tensors[:len(tensors) // 2])


def td3_weights(tensors, device, who="DeviceTD3"):
    """module_params' tensors (or the trained ones: the target fields stay NULL) as an xarm_td3_weights of device pointers"""
    tp = len(tensors) // (6 if len(tensors) in (36, 48) else 3)
    w = _native.XarmTD3Weights()
    for i, t in enumerate(tensors):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
            raise ValueError("%s needs contiguous float32 tensors on %s (tensor %d)" % (who, device, i))
        getattr(w, _native.TD3_TOWERS[i // tp])[i % tp] = t.data_ptr()
    return w


def model_shape(model):
    """(hidden widths of every tower, activation) of a td3.Td3Policy"""
    towers = [getattr(model, name) for name in _native.TD3_TOWERS]
    widths = [tuple(int(m.out_features) for m in t if isinstance(m, torch.nn.Linear))[:-1] for t in towers]
    kinds = {type(m) for t in towers for m in t if not isinstance(m, torch.nn.Linear)}
    act = "tanh" if kinds == {torch.nn.Tanh} else ("relu" if kinds == {torch.nn.ReLU} else None)
    return widths, act


class DeviceTD3:
    """One TD3 step per `update()` call on the model's GPU, and the actor's `act_into` / `predict`.

    model: a td3.Td3Policy whose parameters are contiguous float32 CUDA tensors; they are read and written in place.
    `exp_avg`, `exp_avg_sq` (the trained tensors each: actor, q1, q2) and `step` (int64 [1]: the calls so far) are the state of the torch
    block's two Adams - the critics' has taken `step` steps, the actor's `step // policy_delay`; `stats` [8] = critic_loss, actor_loss,
    mean q1(obs | a_pi), mean y, n_use, actor_stepped, 0, 0 of the last step (actor_loss and the mean q1 keep the last actor step's values);
    `calls` (int64 [1]) counts the stochastic `act_into` calls.  All are device tensors.  act_rows: the most rows an `act_into` call will
    carry (default batch_size): its workspace is sized here (`reserve_act` resizes it).  `launches`: the kernels of one step, a function
    of the depth alone (7 n_hidden + 14), the same on calls with and without an actor step."""

    def __init__(self, model, batch_size, gamma=0.95, lr=1e-3, tau=0.005, policy_delay=2, target_policy_noise=0.2, target_noise_clip=0.5,
                 action_noise=0.1, betas=(0.9, 0.999), eps=1e-8, seed=0, row_offset=0, act_rows=None):
        self.model, self.batch_size, self.seed, self.row_offset = model, int(batch_size), int(seed), int(row_offset)
        self.obs_width, self.act_dim = int(model.actor[0].in_features), int(model.actor[len(model.actor) - 1].out_features)
        widths, act = model_shape(model)
        arch, why = widths[0], None
        if any(w != arch for w in widths) or len(set(arch)) != 1:
            why = "every hidden layer of every tower must have the same width (towers: %s)" % (widths,)
        elif len(arch) not in (2, 3):
            why = "two or three hidden layers (the model has %d)" % len(arch)
        elif arch[0] not in _native.SACW_WIDTHS:
            why = "a hidden width of 64, 128, 192 or 256 (the model's is %d)" % arch[0]
        elif act is None:
            why = "tanh or ReLU between the layers"
        if why is not None:
            raise ValueError("DeviceTD3's kernels need %s.  The torch block (gym_xarm_amd/td3.py td3_step with make_optimizers) runs "
                             "every shape." % why)
        self.hidden, self.n_hidden, self.activation = int(arch[0]), len(arch), act
        self.launches = 7 * self.n_hidden + 14
        self.policy_delay = int(policy_delay)
        self.hyper = dict(gamma=gamma, lr=lr, tau=tau, beta1=betas[0], beta2=betas[1], eps=eps, target_policy_noise=target_policy_noise,
                          target_noise_clip=target_noise_clip, action_noise=action_noise)
        self.device = model.actor[0].weight.device
        if self.device.type != "cuda":
            raise ValueError("DeviceTD3 runs the TD3 step with HIP kernels on the model's GPU: the model is on '%s'.  There is no host path; "
                             "the torch block of train_td3 (gym_xarm_amd/td3.py td3_step: autograd and two Adams) is the host "
                             "implementation." % self.device)
        self._L = _native.load()
        B, D, dev = self.batch_size, self.obs_width, self.device
        nbytes = C.c_int64(0)
        self._layout = self._layout_of(B)
        _native.check(self._L, None, self._L.xarm_td3_workspace_bytes(C.byref(self._layout), C.byref(nbytes)), "xarm_td3_workspace_bytes")
        self._act_work = None
        self.buffers = {"obs": torch.zeros(B, D, device=dev), "next_obs": torch.zeros(B, D, device=dev), "done": torch.zeros(B, device=dev),
                        "use": torch.ones(B, device=dev), "workspace": torch.zeros(max(nbytes.value, 16) // 4, dtype=torch.float32, device=dev)}
        self.exp_avg = [torch.zeros_like(p) for p in trained(self.params())]
        self.exp_avg_sq = [torch.zeros_like(p) for p in trained(self.params())]
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.calls = torch.zeros(1, dtype=torch.int64, device=dev)
        self.stats = torch.zeros(8, device=dev)
        self.num_params = sum(p.numel() for p in trained(self.params()))
        self.reserve_act(act_rows if act_rows is not None else B)

    def params(self):
        return module_params(self.model)

    def reserve_act(self, rows):
        """make the act call's workspace hold `rows` rows (one tensor, kept; a call with more rows than it holds grows it, which
        allocates - reserve before a graph capture)"""
        n = self.n_hidden * rows * self.hidden + self.act_dim * rows + 16
        if self._act_work is None or self._act_work.numel() < n:
            self._act_work = torch.zeros(n, dtype=torch.float32, device=self.device)

    def _layout_of(self, rows):
        return _native.XarmSACWLayout(rows, self.obs_width, self.act_dim, self.hidden, self.n_hidden, _native.SACW_ACTIVATIONS[self.activation],
                                      self.row_offset)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _params(self, hyper, mode="deterministic"):
        return _native.XarmTD3Params(*([self.seed] + [float(hyper[k]) for k in _native.TD3_HYPER] + [self.policy_delay, _native.TD3_MODES[mode]]))

    def _check(self, t, shape, what):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape and t.device == self.device, \
            "%s must be a contiguous float32 %s tensor on the model's device" % (what, list(shape))
        return t

    def _call(self, weights, exp_avg, exp_avg_sq, step, b, hyper, noise_next=None, out_grad=None, out_target=None, out_q=None, out_dqda=None,
              out_stats=None):
        B, D, A = self.batch_size, self.obs_width, self.act_dim
        self._check(b["obs"], (B, D), "obs"); self._check(b["next_obs"], (B, D), "next_obs"); self._check(b["action"], (B, A), "action")
        self._check(b["reward"], (B,), "reward"); self._check(b["done"], (B,), "done")
        for t, shape, k in ((b.get("use"), (B,), "use"), (noise_next, (B, A), "noise_next"), (out_grad, (self.num_params,), "out_grad"),
                            (out_target, (B,), "out_target"), (out_q, (2, B), "out_q"), (out_dqda, (B, A), "out_dqda")):
            if t is not None:
                self._check(t, shape, k)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        W = lambda ts: C.byref(td3_weights(ts, self.device))
        rc = self._L.xarm_td3_update(C.byref(self._layout), C.byref(self._params(hyper)), W(weights), W(exp_avg), W(exp_avg_sq), p(step), p(b["obs"]),
                                     p(b["next_obs"]), p(b["action"]), p(b["reward"]), p(b["done"]), p(b.get("use")), p(noise_next),
                                     p(self.buffers["workspace"]), p(out_grad), p(out_target), p(out_q), p(out_dqda), p(out_stats), self._stream())
        _native.check(self._L, None, rc, "xarm_td3_update")

    def update(self, batch, noise_next=None):
        """one TD3 step on batch = {"obs", "next_obs" [B, D] (flat, normalised), "action" [B, A], "reward", "done" [B], optional "use" [B]}:
        contiguous float32 tensors on the model's device.  The module's parameters and targets, Adam's state and `step` change in place,
        `stats` is rewritten.  noise_next [B, A]: the smoothing noise's standard normals in place of the Philox draw.  No allocation, no
        host read; capturable."""
        self._call(self.params(), self.exp_avg, self.exp_avg_sq, self.step, batch, self.hyper, noise_next, out_stats=self.stats)
        return self.stats

    def update_from(self, buffer, normalize=None, sample=None):
        """sample `buffer` (a DeviceHerReplayBuffer) and step, as DeviceSAC.update_from: `buffer.sample_into`, the two observation triples
        concatenated and normalised by `normalize` (a DeviceVecNormalize; None: concatenated as they are), `ok` as use, then `update`.
        After the first call no allocation and no host read; capturable.
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
                raise ValueError("DeviceTD3: the normaliser's statistics do not belong to this model's observation")
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

    def act_into(self, out, obs, mode="gaussian"):
        """out [E, A] for the normalised flat observation obs [E, D], by mode: "deterministic" tanh(actor(obs)); "gaussian"
        clamp(tanh(actor(obs)) + action_noise z, -1, 1); "uniform" on [-1, 1), obs not read.  Noise: Philox keyed by (seed, row_offset +
        row, calls, column block); a stochastic call advances `calls` on the device.  n_hidden + 2 launches (1 for "uniform"; plus the
        tick).  No allocation, no host read; capturable.  Returns out."""
        E, A = int(obs.shape[0]), self.act_dim
        self._check(obs, (E, self.obs_width), "obs"); self._check(out, (E, A), "out")
        self.reserve_act(E)
        rc = self._L.xarm_td3_act(C.byref(self._layout_of(E)), C.byref(self._params(self.hyper, mode)), C.byref(td3_weights(self.params(), self.device)),
                                  C.c_void_p(self.calls.data_ptr()), C.c_void_p(obs.data_ptr()), C.c_void_p(self._act_work.data_ptr()),
                                  C.c_void_p(out.data_ptr()), self._stream())
        _native.check(self._L, None, rc, "xarm_td3_act")
        return out

    def predict(self, obs):
        """the deployment call: the deterministic action [E, A] for the normalised flat observation (`calls` is left alone)"""
        return self.act_into(torch.empty(int(obs.shape[0]), self.act_dim, device=self.device), obs, "deterministic")

    def grad(self, batch, noise_next=None, lr=0.0, step=None):
        """{"grad" [num_params] (actor's tensors, q1's, q2's), "actor", "critic" (views of it), "dqda" [B, A], "y" [B], "q" [2, B], "stats" [8]} of
        one step on scratch copies of the weights and of Adam's state with lr = 0: the module is not touched (debug; allocates).  step: the
        step count the scratch call starts at (default: one at which the actor steps, policy_delay - 1); on a call without an actor step
        the actor's gradient and dq/da stay zero.  With lr = 0 the q1 at the actor step is the q1 at call start."""
        w = [p.detach().clone() for p in self.params()]
        m, v = [s.clone() for s in self.exp_avg], [s.clone() for s in self.exp_avg_sq]
        dev, B, A = self.device, self.batch_size, self.act_dim
        g, dq, y, q, st = torch.zeros(self.num_params, device=dev), torch.zeros(B, A, device=dev), torch.empty(B, device=dev), \
            torch.empty(2, B, device=dev), torch.zeros(8, device=dev)
        t = torch.full((1,), self.policy_delay - 1 if step is None else int(step), dtype=torch.int64, device=dev)
        self._call(w, m, v, t, batch, dict(self.hyper, lr=float(lr)), noise_next, g, y, q, dq, st)
        na = sum(p.numel() for p in self.params()[:len(w) // 6])
        return {"grad": g, "actor": g[:na], "critic": g[na:], "dqda": dq, "y": y, "q": q, "stats": st}

    def _groups(self):
        ps = trained(self.params())
        tp = len(ps) // 3
        return (("actor", slice(0, tp)), ("critic", slice(tp, 3 * tp))), ps

    def load_optimizer(self, opts):
        """continue from the torch block's Adams, opts = {"actor", "critic"} (td3.make_optimizers): the critics' must have taken n steps and
        the actor's n // policy_delay"""
        groups, ps = self._groups()
        steps = {}
        for k, sl in groups:
            st = torch.zeros(1, dtype=torch.int64, device=self.device)
            load_adam(self.exp_avg[sl], self.exp_avg_sq[sl], st, opts[k], ps[sl])
            steps[k] = int(st.item())
        if steps["actor"] != steps["critic"] // self.policy_delay:
            raise ValueError("the device update keeps one step count: the critics' Adam holds %d steps and the actor's %d, not %d // %d"
                             % (steps["critic"], steps["actor"], steps["critic"], self.policy_delay))
        self.step.fill_(steps["critic"])

    def export_optimizer(self, opts):
        """let the torch block's Adams, built on the same module, continue from this updater's state (reads `step` back): the critics' at
        `step`, the actor's at `step // policy_delay`"""
        groups, ps = self._groups()
        for k, sl in groups:
            st = self.step if k == "critic" else self.step // self.policy_delay
            export_adam(self.exp_avg[sl], self.exp_avg_sq[sl], st, opts[k], ps[sl])
