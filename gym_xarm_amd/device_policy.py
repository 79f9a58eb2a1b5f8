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


class DevicePolicy:
    """`ActorCritic`'s inference on the device: `act`, `act_into`, `predict`.

    model: a train.ActorCritic whose parameters are contiguous float32 CUDA tensors.  Their `data_ptr()`s are read on every
    call, so an in-place optimiser step or `load_state_dict` is seen by the next call with no repacking.  A captured
    torch.cuda.graph bakes the pointers in: the replays keep reading the tensors that were the parameters at capture, so
    update them in place (as torch's optimisers and `load_state_dict` do) and never rebind `param.data` under a live graph.

    Noise is Philox keyed by (seed, row_offset + row, calls, column block): `calls` is a device counter that every stochastic
    call advances behind its kernel, so the replays of a captured graph draw fresh noise, and `row_offset` makes a shard of a
    larger batch draw the noise of its global rows.  A row's result does not depend on the batch it is evaluated in.

    `act_into(out, obs)` runs with no allocation and no host read on the current stream and can be captured."""

    def __init__(self, model, seed=0, row_offset=0):
        self.model, self.seed, self.row_offset = model, int(seed), int(row_offset)
        self.obs_width = int(model.pi[0].in_features)
        self.act_dim = int(model.pi[4].out_features)
        if int(model.pi[0].out_features) != _native.POLICY_HIDDEN or int(model.pi[2].out_features) != _native.POLICY_HIDDEN:
            raise ValueError("DevicePolicy evaluates 64-64 towers (XARM_POLICY_HIDDEN)")
        if self.obs_width > _native.POLICY_MAX_DIM or not 1 <= self.act_dim <= _native.POLICY_MAX_ACT:
            raise ValueError("DevicePolicy: observation width %d (<= %d) / action width %d (1..%d) out of range"
                             % (self.obs_width, _native.POLICY_MAX_DIM, self.act_dim, _native.POLICY_MAX_ACT))
        self.device = model.log_std.device
        self._L = self.calls = None
        if self.device.type == "cuda":
            self._lib()

    def _lib(self):
        if self._L is None:
            if self.device.type != "cuda":
                raise ValueError("DevicePolicy evaluates the policy with a HIP kernel on the model's GPU: the model is on '%s'.  There "
                                 "is no host path; train.ActorCritic is the torch implementation." % self.device)
            self._L = _native.load()
            self.calls = torch.zeros(1, dtype=torch.int64, device=self.device)    # stochastic calls so far
        return self._L

    def _params(self):
        m = self.model
        return (m.pi[0].weight, m.pi[0].bias, m.pi[2].weight, m.pi[2].bias, m.pi[4].weight, m.pi[4].bias,
                m.vf[0].weight, m.vf[0].bias, m.vf[2].weight, m.vf[2].bias, m.vf[4].weight, m.vf[4].bias, m.log_std)

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
        """One launch (plus the counter tick of a stochastic call) on the current stream: out["action"] [E, A], out["env_action"]
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
        layout = _native.XarmPolicyLayout(E, od, gd, A, _native.POLICY_HIDDEN, self.row_offset)
        stats, clip, eps = None, 10.0, 1e-8
        if normalize is not None:
            if int(normalize.dim) != self.obs_width or normalize.stats.device != self.device:
                raise ValueError("DevicePolicy: the normaliser's statistics do not belong to this model's observation")
            stats, clip, eps = C.c_void_p(normalize.stats.data_ptr()), float(normalize.clip_obs), float(normalize.eps)
        params = _native.XarmPolicyParams(self.seed, clip, eps, 1 if deterministic else 0)
        p = lambda k: C.c_void_p(out[k].data_ptr()) if k in out else None
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
