"""ctypes view of tests/hostbuild_a2c (g++ -ffp-contract=off build of csrc/xarm_a2c_core.h) - CPU-side tests only - with the batches,
the torch reference - train.py's a2c_loss and a2c_update on float32 and float64 copies of the model - and the tolerance rule that the
host and GPU tests of the A2C update share.  Models and rows come from policy_host.case."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import policy_host as PH
from gym_xarm_amd import train as TR

ROOT = PH.ROOT
DIR = os.path.join(ROOT, "tests", "hostbuild_a2c")
HYPER = ("gamma", "lr", "alpha", "eps", "vf_coef", "ent_coef", "max_grad_norm")
DEFAULTS = dict(gamma=0.99, lr=7e-4, alpha=0.99, eps=1e-5, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5)
WIDTHS = ((14, 4), (29, 1), (30, 4), (96, 16))          # Reach, an odd width, PickAndPlace, the maximum
SHAPES = ((1, 1), (1, 31), (5, 13), (5, 200))           # T x E: one row, under a tile, two full tiles and one row, 1000 rows
_lib = None
_refs = {}


def sources():
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    return [os.path.join(DIR, "a2c_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + \
        [os.path.join(csrc, h) for h in ("xarm_a2c_core.h", "xarm_opt_core.h", "xarm_policy_core.h", "xarm_norm_core.h", "xarm_core.h")]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "liba2c_host.so")
    srcs = sources()
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + PH.gxx_flags() + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.ah_workspace_bytes.argtypes = L.ah_param_count.argtypes = [vp]
    L.ah_workspace_bytes.restype = L.ah_param_count.restype = C.c_int64
    L.ah_geometry.argtypes = [vp, vp]
    L.ah_update.argtypes = [vp] * 14
    _lib = L
    return L


def hyper(**kw):
    h = dict(DEFAULTS)
    h.update(kw)
    return h


def abi_params(h):
    from gym_xarm_amd import _native
    return _native.XarmA2CParams(*[float(h[k]) for k in HYPER])


def abi_layout(T, E, D, A):
    from gym_xarm_amd import _native
    return _native.XarmA2CLayout(E, T, D, A, 64)


def geometry(T, E, D, A):
    """(tiles, groups, rows per tile, the most groups) of the gradient kernel's launch for this layout"""
    out = np.zeros(4, np.int64)
    lib().ah_geometry(C.byref(abi_layout(T, E, D, A)), C.c_void_p(out.ctypes.data))
    return [int(v) for v in out]


def sizes(D, A):
    return [64 * D, 64, 4096, 64, 64 * A, A, 64 * D, 64, 4096, 64, 64, 1, A]


def split(flat, D, A):
    """the 13 tensors of a flat [P] array"""
    o = np.cumsum([0] + sizes(D, A))
    return [flat[o[i]:o[i + 1]] for i in range(13)]


def flat_of(w):
    return np.concatenate([np.asarray(w[k], np.float64).ravel() for k in PH.NAMES])


def zeros_like_weights(w):
    return {k: PH.aligned(np.zeros_like(w[k])) for k in PH.NAMES}


def clone_weights(w):
    return {k: PH.aligned(w[k]) for k in PH.NAMES}


def make_batch(D, A, T, E, scale, masked=True, seed=0, reward_scale=1.0):
    """rows of policy_host.case (uniform in [-10, 10] is far outside what VecNormalize hands on: scaled to [-2.5, 2.5]), standard
    normal actions and rewards, 10 % episode ends, a use mask with about 10 % zeros"""
    N = T * E
    rs = np.random.RandomState(1000 * seed + 7 * D + A + 131 * N)
    if N + E <= PH.ROWS:
        rows = PH.case(D, 0, A, scale)["rows"] * np.float32(0.25)
    else:
        rows = rs.uniform(-2.5, 2.5, (N + E, D)).astype(np.float32)
    b = {"obs": np.ascontiguousarray(rows[:N].reshape(T, E, D)), "last_obs": np.ascontiguousarray(rows[N:N + E]),
         "action": rs.standard_normal((T, E, A)).astype(np.float32), "reward": (reward_scale * rs.standard_normal((T, E))).astype(np.float32),
         "done": (rs.uniform(size=(T, E)) < 0.1).astype(np.float32),
         "use": (rs.uniform(size=(T, E)) >= 0.1).astype(np.float32) if masked else None}
    return b


def model_of(D, A, scale):
    """a private copy of policy_host.case's model (the tests update it)"""
    return copy.deepcopy(PH.case(D, 0, A, scale)["model"])


def host_update(w, sq, b, h):
    """one update of the host build, in place on the aligned arrays of w and sq; returns (rc, {"returns", "grad", "stats"})"""
    T, E, D = b["obs"].shape
    A = b["action"].shape[2]
    from gym_xarm_amd import _native
    layout, params = abi_layout(T, E, D, A), abi_params(h)
    ws, qs = _native.XarmPolicyWeights(*[w[k].ctypes.data for k in PH.NAMES]), _native.XarmPolicyWeights(*[sq[k].ctypes.data for k in PH.NAMES])
    out = {"returns": np.full((T, E), np.nan, np.float32), "grad": np.full(sum(sizes(D, A)), np.nan, np.float32), "stats": np.full(8, np.nan, np.float32)}
    work = PH.aligned(np.zeros(4, np.float32))
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    rc = lib().ah_update(C.byref(layout), C.byref(params), C.byref(ws), C.byref(qs), p(b["obs"]), p(b["action"]), p(b["reward"]), p(b["done"]),
                         p(b["use"]), p(b["last_obs"]), p(work), *[p(out[k]) for k in ("returns", "grad", "stats")])
    return rc, out


# ---- torch: train.py's own update functions on the batch, in the model's dtype
def rollout_of(b, dt):
    """(the rollout dict of train.py's update functions, last_obs) of a NumPy batch"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)
    r = {k: t(b[k]) for k in ("obs", "action", "reward", "done")}
    r["use"] = torch.ones_like(r["reward"]) if b["use"] is None else t(b["use"])
    return r, t(b["last_obs"])


def torch_loss(model, b, h):
    rollout, last = rollout_of(b, model.log_std.dtype)
    loss, rets, t = TR.a2c_loss(model, rollout, last, h["gamma"], h["vf_coef"], h["ent_coef"])
    st = {k: float(t[k].detach()) for k in ("policy_loss", "value_loss", "entropy", "n_use")}
    st["policy_abs"] = float((t["adv"] * t["logp"].detach() * t["use"]).abs().sum() / t["n_use"])
    return loss, rets, st


def torch_grad(model, b, h, dtype):
    """(flat gradient float64 [P], returns [T, E], stats) of a `dtype` copy of the model"""
    m = copy.deepcopy(model).to(dtype)
    loss, rets, st = torch_loss(m, b, h)
    loss.backward()
    g = np.concatenate([p.grad.detach().numpy().astype(np.float64).ravel() for p in PH.model_params(m)])
    st["grad_norm"] = float(np.sqrt((g * g).sum()))
    return g, rets.numpy(), st


def torch_updates(model, batches, h, dtype):
    """clip_grad_norm_ + RMSprop.step over the batches on a `dtype` copy; returns (model, optimiser)"""
    m = copy.deepcopy(model).to(dtype)
    opt = torch.optim.RMSprop(m.parameters(), lr=h["lr"], alpha=h["alpha"], eps=h["eps"])
    for b in batches:
        TR.a2c_update(m, opt, *rollout_of(b, dtype), h["gamma"], h["vf_coef"], h["ent_coef"], h["max_grad_norm"])
    return m, opt


def reference(D, A, T, E, scale, ent_coef, masked=True):
    """the batch, the float64 and float32 torch gradients and the yardstick of one case; computed once and only read"""
    key = (D, A, T, E, scale, ent_coef, masked)
    if key not in _refs:
        h = hyper(ent_coef=ent_coef)
        b = make_batch(D, A, T, E, scale, masked)
        model = PH.case(D, 0, A, scale)["model"]
        g64, ret64, st64 = torch_grad(model, b, h, torch.float64)
        g32, _, _ = torch_grad(model, b, h, torch.float32)
        _refs[key] = dict(h=h, b=b, g64=g64, g32=g32, ret64=ret64, st64=st64, Y=yardstick(g32, g64, D, A))
    return _refs[key]


# ---- the rule: per tensor, max|g - g64| <= 4 Y max|g64_tensor| + 2^-23 max|g64_model|, Y = what torch's float32 loses
def yardstick(x32, x64, D, A):
    y = 0.0
    for a, r in zip(split(np.asarray(x32, np.float64), D, A), split(x64, D, A)):
        m = np.abs(r).max()
        if m > 0.0:
            y = max(y, np.abs(a - r).max() / m)
    return y


def bounds(x64, Y, D, A):
    """the rule's bound of every tensor"""
    floor = 2.0 ** -23 * np.abs(x64).max()
    return [4.0 * Y * np.abs(r).max() + floor for r in split(x64, D, A)]


def rule(x, x64, Y, D, A, keep=None):
    """(worst error / bound over the tensors, worst error relative to the tensor's largest entry in units of Y).  keep: bool [P],
    the entries compared"""
    worst, in_y = 0.0, 0.0
    keep = np.ones(x64.shape, bool) if keep is None else keep
    for a, r, k, bd in zip(split(np.asarray(x, np.float64), D, A), split(x64, D, A), split(keep, D, A), bounds(x64, Y, D, A)):
        if not k.any():
            continue
        err = np.abs(a - r)[k].max()
        worst = max(worst, err / bd if bd > 0 else (0.0 if err == 0 else np.inf))
        if np.abs(r).max() > 0 and Y > 0:
            in_y = max(in_y, err / np.abs(r).max() / Y)
    return worst, in_y


def worst_tensor(x, x64, D, A):
    """(name, size of that tensor's largest float64 entry relative to the model's) of the tensor with the largest error relative to
    its own largest entry - for the record the tests print"""
    rel = [np.abs(a - r).max() / np.abs(r).max() if np.abs(r).max() > 0 else 0.0 for a, r in zip(split(np.asarray(x, np.float64), D, A), split(x64, D, A))]
    i = int(np.argmax(rel))
    return PH.NAMES[i], np.abs(split(x64, D, A)[i]).max() / np.abs(x64).max()


def sensitive(g64, Y, D, A):
    """bool [P]: gradient entries within the gradient rule's bound of zero - RMSprop's first step is nearly lr 10 sign(g), so their
    parameters are left out of the parameter comparison (at most 1 % of a tensor's entries may be)"""
    out = []
    for r, bd in zip(split(g64, D, A), bounds(g64, Y, D, A)):
        out.append(np.abs(r) <= bd)
    return np.concatenate(out)
