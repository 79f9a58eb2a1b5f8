"""Device-resident A2C update: train.a2c_update - bootstrap value, n-step returns, the backward of both towers,
`clip_grad_norm_` and `RMSprop.step` - as one stream-ordered call of six HIP launches (csrc/xarm_k_a2c.hip).

The torch update of train.py runs on the order of a hundred small launches per update: a second forward of both towers over
n_steps x num_envs rows under autograd, the backward, the clip and the optimiser.  `DeviceA2C` keeps the rollout in the buffers
`train.TorchA2C` uses and updates the module's own parameter tensors in place, so a `DevicePolicy` on the same module (or the
module itself) sees the new weights in its next call.  The checker is train.a2c_loss / a2c_update, the functions train() itself
runs without device_update: tests/a2c_host.py calls them on float64 and float32 copies of the model (tests/test_a2c_host.py,
tests/test_a2c_gpu.py).

With `wide=True` the same update runs as a chain of per-layer f32 MFMA GEMM launches (csrc/xarm_k_a2cw.hip) for
equal-width towers of two or three hidden layers of 64, 128, 192 or 256 units, tanh or ReLU - the reference's
`net_arch=[256, 256, 256]` among them (tests/test_a2cw_host.py, tests/test_a2cw_gpu.py)."""
import ctypes as C

import torch

from . import _native
from .device_policy import is_tile64, tower_params, tower_shape, wide_supported
from .train import rollout_buffers, store_rollout  # noqa: F401  (store_rollout is re-exported)

HYPER = ("gamma", "lr", "alpha", "eps", "vf_coef", "ent_coef", "max_grad_norm")


def module_params(model):
    """the 13 parameter tensors of a train.ActorCritic in the order of include/xarm_hip.h xarm_policy_weights"""
    m = model
    return (m.pi[0].weight, m.pi[0].bias, m.pi[2].weight, m.pi[2].bias, m.pi[4].weight, m.pi[4].bias,
            m.vf[0].weight, m.vf[0].bias, m.vf[2].weight, m.vf[2].bias, m.vf[4].weight, m.vf[4].bias, m.log_std)


def load_square_avg(square_avg, opt, params):
    """copy the `square_avg` state of a torch.optim.RMSprop built on `params` into the 13 state tensors (zeros for a parameter the
    optimiser has not stepped yet).  Momentum and centred RMSprop have state the device update does not carry: refused."""
    for g in opt.param_groups:
        if g.get("momentum", 0) != 0 or g.get("centered", False) or g.get("weight_decay", 0) != 0:
            raise ValueError("the device update is RMSprop without momentum, centring or weight decay")
    with torch.no_grad():
        for s, p in zip(square_avg, params):
            st = opt.state.get(p, {})
            if "square_avg" in st:
                s.copy_(st["square_avg"])
            else:
                s.zero_()


def export_square_avg(square_avg, opt, params):
    """the other direction: the optimiser continues from the 13 state tensors.  A parameter the optimiser has not stepped yet gets
    the state RMSprop itself would create (its `step` counter, which RMSprop keeps and never reads, starts at 0)."""
    with torch.no_grad():
        for s, p in zip(square_avg, params):
            st = opt.state[p]
            if "square_avg" in st:
                st["square_avg"].copy_(s)
            else:
                st["step"] = torch.zeros((), dtype=torch.float32)
                st["square_avg"] = s.detach().clone()


def policy_weights(tensors, device, who):
    """the 13 tensors as an xarm_policy_weights of device pointers"""
    w = _native.XarmPolicyWeights()
    for k, t in zip(_native.POLICY_WEIGHT_FIELDS, tensors):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
            raise ValueError("%s needs contiguous float32 tensors on %s (%s)" % (who, device, k))
        setattr(w, k, t.data_ptr())
    return w


def acw_weights(tensors, device, who):
    """pi's tensors, vf's and log_std (tower_params' order) as an xarm_acw_weights of device pointers"""
    tp = (len(tensors) - 1) // 2
    w = _native.XarmACWWeights()
    for i, t in enumerate(tensors):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
            raise ValueError("%s needs contiguous float32 tensors on %s (tensor %d)" % (who, device, i))
        if i == 2 * tp:
            w.log_std = t.data_ptr()
        else:
            (w.pi if i < tp else w.vf)[i % tp] = t.data_ptr()
    return w


class DeviceA2C:
    """One A2C update per `update()` call on the model's GPU.

    model: a train.ActorCritic whose parameters are contiguous float32 CUDA tensors; they are read and written in place.
    `buffers`: obs [T, E, D], action [T, E, A], reward / done / use [T, E] and the workspace, allocated once; slice k of each is
    contiguous, so `DevicePolicy.act_into` can write `buffers["action"][k]` directly.  `square_avg`: RMSprop's 13 state tensors.
    `update(last_obs)` allocates nothing and reads nothing back, so it can be captured in a torch.cuda.graph; `stats` is the device
    tensor [policy_loss, value_loss, entropy, grad_norm, n_use, 0, 0, 0] of the last update.

    `backend`: "tile64" - the fused 64-row tile of DESIGN.md 21, six launches, for a 64-64 tanh model - or "wide" - the per-layer MFMA GEMM
    chain of DESIGN.md 26 (csrc/xarm_k_a2cw.hip), 3 L + 7 launches with L hidden layers, for equal widths of 64, 128, 192 or 256 units in
    two or three layers, tanh or ReLU.  "wide" is opt-in: wide None or False is "tile64" and refuses every other shape; wide=True is "wide"
    for every supported shape, 64-64 tanh included.  On "wide", `params()` and `square_avg` hold one tensor per parameter in the flat order
    of out_grad: pi's tensors, vf's, log_std; its workspace holds every layer's activations and deltas of all n_steps x num_envs rows.
    `launches`: the kernels of one update."""

    def __init__(self, model, num_envs, n_steps=5, gamma=0.99, lr=7e-4, alpha=0.99, eps=1e-5, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5,
                 wide=None):
        self.model, self.num_envs, self.n_steps = model, int(num_envs), int(n_steps)
        self.hyper = dict(gamma=gamma, lr=lr, alpha=alpha, eps=eps, vf_coef=vf_coef, ent_coef=ent_coef, max_grad_norm=max_grad_norm)
        self.obs_width = int(model.pi[0].in_features)
        self.act_dim = int(model.pi[-1].out_features)
        self.widths, self.activation = tower_shape(model)
        self.backend = "wide" if wide else "tile64"
        if self.backend == "tile64" and not is_tile64(model):
            raise ValueError("DeviceA2C updates 64-64 tanh towers (XARM_POLICY_HIDDEN), not %s %s (pass wide=True for equal widths of 64, 128, "
                             "192 or 256 in 2 or 3 layers, tanh or relu); train.a2c_update is the torch implementation for every other shape"
                             % tuple(map(str, tower_shape(model))))
        if self.backend == "wide" and not wide_supported(model):
            raise ValueError("DeviceA2C(wide=True) updates equal-width towers of 2 or 3 hidden layers of 64, 128, 192 or 256 units, tanh or relu, not "
                             "%s %s; train.a2c_update is the torch implementation for every other shape" % (list(self.widths), self.activation))
        self.device = model.log_std.device
        if self.device.type != "cuda":
            raise ValueError("DeviceA2C runs the update with HIP kernels on the model's GPU: the model is on '%s'.  There is no host "
                             "path; the torch update of train.py (autograd, clip_grad_norm_, RMSprop) is the host implementation." % self.device)
        self._L = _native.load()
        T, E, D, A, dev = self.n_steps, self.num_envs, self.obs_width, self.act_dim, self.device
        nbytes = C.c_int64(0)
        if self.backend == "wide":
            L = len(self.widths)
            self._layout = _native.XarmA2CWLayout(E, T, D, A, self.widths[0], L, _native.SACW_ACTIVATIONS[self.activation])
            _native.check(self._L, None, self._L.xarm_a2cw_workspace_bytes(C.byref(self._layout), C.byref(nbytes)), "xarm_a2cw_workspace_bytes")
            self.launches = 3 * L + 7
        else:
            self._layout = _native.XarmA2CLayout(E, T, D, A, _native.POLICY_HIDDEN)
            _native.check(self._L, None, self._L.xarm_a2c_workspace_bytes(C.byref(self._layout), C.byref(nbytes)), "xarm_a2c_workspace_bytes")
            self.launches = 6
        self.buffers = rollout_buffers(T, E, D, A, dev, nbytes.value)
        self.square_avg = [torch.zeros_like(p) for p in self.params()]
        self.stats = torch.zeros(8, device=dev)
        self.num_params = sum(p.numel() for p in self.params())

    def params(self):
        """the trained tensors in the flat order of out_grad: the 13 of xarm_policy_weights on "tile64"; pi's W1, b1, ..., vf's, log_std on "wide"."""
        if self.backend == "wide":
            pi, vf = tower_params(self.model)
            return pi + vf + (self.model.log_std,)
        return module_params(self.model)

    def _weights(self, tensors):
        if self.backend == "wide":
            return acw_weights(tensors, self.device, "DeviceA2C")
        return policy_weights(tensors, self.device, "DeviceA2C")

    def set_hyper(self, **kw):
        """rewrite entries of `hyper` (lr, ...): the next update reads them"""
        for k, v in kw.items():
            if k not in self.hyper:
                raise KeyError("DeviceA2C has no hyper-parameter %r (it has %s)" % (k, ", ".join(sorted(self.hyper))))
            self.hyper[k] = v

    def store(self, k, obs, action, reward, done, resetting=None):
        """slot k of the rollout (train.store_rollout)"""
        store_rollout(self.buffers, k, obs, action, reward, done, resetting)

    def _call(self, weights, square_avg, last_obs, hyper, out_returns, out_grad, out_stats):
        E, D = self.num_envs, self.obs_width
        assert last_obs.dtype == torch.float32 and last_obs.is_contiguous() and tuple(last_obs.shape) == (E, D) and last_obs.device == self.device, \
            "last_obs must be a contiguous float32 [num_envs, D] tensor on the model's device"
        b = self.buffers
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        params = _native.XarmA2CParams(*[float(hyper[k]) for k in HYPER])
        name = "xarm_a2cw_update" if self.backend == "wide" else "xarm_a2c_update"
        ws, sq = self._weights(weights), self._weights(square_avg)          # held until the call has returned
        rc = getattr(self._L, name)(C.byref(self._layout), C.byref(params), C.byref(ws), C.byref(sq),
                                    p(b["obs"]), p(b["action"]), p(b["reward"]), p(b["done"]), p(b["use"]), p(last_obs), p(b["workspace"]),
                                    p(out_returns), p(out_grad), p(out_stats), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        _native.check(self._L, None, rc, name)

    def update(self, last_obs, out_returns=None, out_grad=None):
        """one update from the stored rollout and the observation after its last step; the module's parameters and `square_avg`
        change in place, `stats` is rewritten.  out_returns [T, E] / out_grad [num_params] (debug): filled with the returns and with
        the gradient before the clip.  No allocation, no host read; capturable."""
        self._call(self.params(), self.square_avg, last_obs, self.hyper, out_returns, out_grad, self.stats)
        return self.stats

    def grad(self, last_obs):
        """(flat gradient before the clip [num_params], returns [T, E], stats [8]) of the stored rollout, computed by the same call on
        a scratch copy of the weights and of square_avg with lr = 0: the module is not touched (debug; allocates)"""
        w, sq = [p.detach().clone() for p in self.params()], [s.clone() for s in self.square_avg]
        g, r, st = torch.empty(self.num_params, device=self.device), torch.empty(self.n_steps, self.num_envs, device=self.device), torch.zeros(8, device=self.device)
        self._call(w, sq, last_obs, dict(self.hyper, lr=0.0), r, g, st)
        return g, r, st

    def load_optimizer(self, opt):
        """continue from a torch.optim.RMSprop built on the same module"""
        load_square_avg(self.square_avg, opt, self.params())

    def export_optimizer(self, opt):
        """let a torch.optim.RMSprop built on the same module continue from this updater's state"""
        export_square_avg(self.square_avg, opt, self.params())
