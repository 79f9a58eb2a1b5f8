"""Device-resident MlpPolicy: the forward of train.py's `ActorCritic` - mean, Gaussian sample, clamp, log-probability and value -
as one fused HIP launch per call (csrc/xarm_k_policy.hip).

The rollout of train.py evaluates `model.dist(obs).sample().clamp(-1, 1)` (and, once per update, `model.value(obs)`) as a chain
of small torch launches: six GEMMs, four tanh, an exp, a normal sample, a clamp.  `DevicePolicy` reads the module's own parameter
tensors in place and produces action, clamped action, log-probability and value in one kernel on the f32 MFMA, followed by a
one-thread launch that advances the noise counter.  `ActorCritic`, the torch rollout and the torch update stay as they are and
are the checker (tests/test_policy_host.py, tests/test_policy_gpu.py); nothing here computes a gradient.
"""
import ctypes as C

import torch

from . import _native


def tower_shape(model):
    """(hidden widths, activation) of a train.ActorCritic, read off `pi`'s Linear layers and the recorded `activation`"""
    linears = [m for m in model.pi if isinstance(m, torch.nn.Linear)]
    return tuple(int(m.out_features) for m in linears[:-1]), str(getattr(model, "activation", "tanh"))


def is_tile64(model):
    """the 64-64 tanh shape of the fused kernels (xarm_policy_act, xarm_a2c_update, xarm_ppo_update)"""
    return tower_shape(model) == ((_native.POLICY_HIDDEN, _native.POLICY_HIDDEN), "tanh")


def wide_supported(model):
    widths, activation = tower_shape(model)
    return (len(widths) in (2, _native.SACW_MAX_LAYERS) and len(set(widths)) == 1 and widths[0] in _native.SACW_WIDTHS
            and activation in _native.SACW_ACTIVATIONS)


def tower_params(model):
    """(pi's tensors W1, b1, ..., W_out, b_out; vf's) of a train.ActorCritic of any depth"""
    return tuple(tuple(t for m in tower if isinstance(m, torch.nn.Linear) for t in (m.weight, m.bias)) for tower in (model.pi, model.vf))


class DevicePolicy:
    """`ActorCritic`'s inference on the device: `act`, `act_into`, `predict`.

    `backend`: "tile64" - the fused kernel of DESIGN.md 20, one launch, for a 64-64 tanh model - or "wide" - a layer-by-layer forward on
    the f32 MFMA GEMM kernel of the wide SAC (csrc/xarm_k_acw.hip), n_hidden + 3 launches, for equal widths of 64, 128,
    192 or 256 units in two or three layers, tanh or ReLU.  wide None: "tile64" for a 64-64 tanh model and "wide" for every other
    supported shape; wide=True forces "wide".  act_rows: the most rows a call will carry on the wide backend (default 0: the first call
    sizes it) - its activations live in ONE workspace tensor; `reserve_act(rows)` sizes it before a capture.

    model: a train.ActorCritic whose parameters are contiguous float32 CUDA tensors.  Their `data_ptr()`s are read on every
    call, so an in-place optimiser step or `load_state_dict` is seen by the next call with no repacking.  A captured
    torch.cuda.graph bakes the pointers in: the replays keep reading the tensors that were the parameters at capture, so
    update them in place (as torch's optimisers and `load_state_dict` do) and never rebind `param.data` under a live graph.

    Noise is Philox keyed by (seed, row_offset + row, calls, column block): `calls` is a device counter that every stochastic
    call advances behind its kernel, so the replays of a captured graph draw fresh noise, and `row_offset` makes a shard of a
    larger batch draw the noise of its global rows.  A row's result does not depend on the batch it is evaluated in.

    `act_into(out, obs)` runs with no allocation and no host read on the current stream and can be captured."""

    def __init__(self, model, seed=0, row_offset=0, wide=None, act_rows=None):
        self.model, self.seed, self.row_offset = model, int(seed), int(row_offset)
        self.obs_width = int(model.pi[0].in_features)
        self.act_dim = int(model.pi[-1].out_features)
        self.widths, self.activation = tower_shape(model)
        if wide is False and not is_tile64(model):
            raise ValueError("DevicePolicy: the fused kernel (wide=False) evaluates 64-64 tanh towers (XARM_POLICY_HIDDEN), not %s %s"
                             % (list(self.widths), self.activation))
        self.backend = "tile64" if is_tile64(model) and not wide else "wide"
        if self.backend == "wide" and not wide_supported(model):
            raise ValueError("DevicePolicy evaluates 64-64 tanh towers (the fused kernel) and equal-width towers of 2 or 3 hidden layers of 64, 128, 192 or 256 units, tanh or relu, "
                             "not %s %s; ActorCritic.dist is the torch implementation for every other shape" % (list(self.widths), self.activation))
        if self.obs_width > _native.POLICY_MAX_DIM or not 1 <= self.act_dim <= _native.POLICY_MAX_ACT:
            raise ValueError("DevicePolicy: observation width %d (<= %d) / action width %d (1..%d) out of range"
                             % (self.obs_width, _native.POLICY_MAX_DIM, self.act_dim, _native.POLICY_MAX_ACT))
        self.device = model.log_std.device
        self._L = self.calls = self._act_work = None
        self._act_rows = 0
        if self.device.type == "cuda":
            self._lib()
            if self.backend == "wide" and act_rows:
                self.reserve_act(act_rows)

    def _lib(self):
        if self._L is None:
            if self.device.type != "cuda":
                raise ValueError("DevicePolicy evaluates the policy with a HIP kernel on the model's GPU: the model is on '%s'.  There "
                                 "is no host path; train.ActorCritic is the torch implementation." % self.device)
            self._L = _native.load()
            self.calls = torch.zeros(1, dtype=torch.int64, device=self.device)    # stochastic calls so far
        return self._L

    def _params(self):
        pi, vf = tower_params(self.model)
        return pi + vf + (self.model.log_std,)

    def _wide_layout(self, rows, od, gd):
        return _native.XarmACWLayout(int(rows), od, gd, self.act_dim, self.widths[0], len(self.widths), _native.SACW_ACTIVATIONS[self.activation],
                                     self.row_offset)

    def reserve_act(self, rows):
        """wide backend: make the act call's workspace hold `rows` rows (one tensor, kept; a call with more rows than it holds grows it,
        which allocates - reserve before a capture)"""
        if self.backend != "wide" or int(rows) <= self._act_rows:
            return
        L, nbytes = self._lib(), C.c_int64(0)
        _native.check(L, None, L.xarm_acw_workspace_bytes(C.byref(self._wide_layout(rows, self.obs_width, 0)), C.byref(nbytes)), "xarm_acw_workspace_bytes")
        self._act_work = torch.zeros(max(nbytes.value, 16) // 4, dtype=torch.float32, device=self.device)
        self._act_rows = int(rows)

    def _wide_weights(self):
        pi, vf = tower_params(self.model)
        w = _native.XarmACWWeights()
        for name, ts in (("pi", pi), ("vf", vf)):
            for i, t in enumerate(ts):
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                    raise ValueError("DevicePolicy needs contiguous float32 parameters on %s (%s[%d])" % (self.device, name, i))
                getattr(w, name)[i] = t.data_ptr()
        w.log_std = self.model.log_std.data_ptr()
        return w

    def _weights(self):
        w = _native.XarmPolicyWeights()
        for k, t in zip(_native.POLICY_WEIGHT_FIELDS, self._params()):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("DevicePolicy needs contiguous float32 parameters on %s (%s)" % (self.device, k))
            setattr(w, k, t.data_ptr())
        return w

    def _parts(self, obs):
        """(obs_dim, goal_dim, num_envs, the three row pointers) of the env's dict, a flat tensor, or an [E, D] row set"""
        parts = [obs["observation"], obs["achieved_goal"], obs["desired_goal"]] if isinstance(obs, dict) else [obs]
        E = int(parts[0].shape[0])
        for x in parts:
            assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 2 and x.shape[0] == E and x.device == self.device, \
                "observation parts must be contiguous float32 [num_envs, dim] tensors on the model's device"
        od, gd = int(parts[0].shape[1]), int(parts[1].shape[1]) if len(parts) == 3 else 0
        if len(parts) == 3 and int(parts[2].shape[1]) != gd or od + 2 * gd != self.obs_width:
            raise ValueError("DevicePolicy: the observation is %d + 2 x %d wide, the model takes %d" % (od, gd, self.obs_width))
        return od, gd, E, [C.c_void_p(x.data_ptr()) for x in parts] + [None] * (3 - len(parts))

    def alloc_out(self, num_envs):
        """the tensors act_into fills"""
        E, dev = int(num_envs), self.device
        return {"action": torch.empty(E, self.act_dim, device=dev), "env_action": torch.empty(E, self.act_dim, device=dev),
                "logp": torch.empty(E, device=dev), "value": torch.empty(E, device=dev)}

    def act_into(self, out, obs, deterministic=False, normalize=None):
        """One launch (n_hidden + 3 on the wide backend; plus the counter tick of a stochastic call) on the current stream: out["action"] [E, A], out["env_action"]
        (clamped to [-1, 1]: what env.step takes), and, where the dict has them, out["logp"] [E] and out["value"] [E] (leave
        "value" out and the value tower is not evaluated).  obs: the env's dict, the flat tensor of a 'NoGoal' env, or an
        already normalised [E, D] tensor.  normalize: a DeviceVecNormalize whose statistics, frozen, normalise the raw
        observation inside the kernel.  No allocation, no host read; capturable."""
        L = self._lib()
        od, gd, E, parts = self._parts(obs)
        A = self.act_dim
        for k, shape in (("action", (E, A)), ("env_action", (E, A)), ("logp", (E,)), ("value", (E,))):
            if k in out:
                assert out[k].dtype == torch.float32 and out[k].is_contiguous() and out[k].shape == shape and out[k].device == self.device, k
        stats, clip, eps = None, 10.0, 1e-8
        if normalize is not None:
            if int(normalize.dim) != self.obs_width or normalize.stats.device != self.device:
                raise ValueError("DevicePolicy: the normaliser's statistics do not belong to this model's observation")
            stats, clip, eps = C.c_void_p(normalize.stats.data_ptr()), float(normalize.clip_obs), float(normalize.eps)
        params = _native.XarmPolicyParams(self.seed, clip, eps, 1 if deterministic else 0)
        p = lambda k: C.c_void_p(out[k].data_ptr()) if k in out else None
        if self.backend == "wide":
            self.reserve_act(E)
            rc = L.xarm_acw_act(C.byref(self._wide_layout(E, od, gd)), C.byref(params), C.byref(self._wide_weights()), stats,
                                C.c_void_p(self.calls.data_ptr()), *parts, C.c_void_p(self._act_work.data_ptr()), p("action"), p("env_action"),
                                p("logp"), p("value"), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
            _native.check(L, None, rc, "xarm_acw_act")
            return out
        layout = _native.XarmPolicyLayout(E, od, gd, A, _native.POLICY_HIDDEN, self.row_offset)
        rc = L.xarm_policy_act(C.byref(layout), C.byref(params), C.byref(self._weights()), stats, C.c_void_p(self.calls.data_ptr()),
                               *parts, p("action"), p("env_action"), p("logp"), p("value"),
                               C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _native.check(L, None, rc, "xarm_policy_act")
        return out

    def act(self, obs, deterministic=False, normalize=None):
        """{"action", "env_action", "logp", "value"} for one batch of observations"""
        E = int((obs["observation"] if isinstance(obs, dict) else obs).shape[0])
        return self.act_into(self.alloc_out(E), obs, deterministic, normalize)

    def predict(self, obs, deterministic=True, normalize=None):
        """the deployment call (benchmark/display.py: VecNormalize.load, training = False, model.predict(obs, deterministic=True)):
        the clamped action for the env's raw observation, normalised in the kernel with `normalize`'s frozen statistics"""
        E = int((obs["observation"] if isinstance(obs, dict) else obs).shape[0])
        out = {"action": torch.empty(E, self.act_dim, device=self.device), "env_action": torch.empty(E, self.act_dim, device=self.device)}
        return self.act_into(out, obs, deterministic, normalize)["env_action"]
