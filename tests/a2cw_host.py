"""ctypes view of tests/hostbuild_a2cw (g++ -ffp-contract=off build of csrc/xarm_a2cw_core.h) - CPU-side tests only - with the torch
reference that the host and GPU tests of the wide A2C update share.  Models, batches, `settle` and the rule (yardstick, bounds, rule,
sensitive) are ppow_host's; the reference is train.py's own a2c_loss / a2c_update on float64 and float32 copies of the same
ActorCritic(net_arch, activation), reached through a2c_host's helpers.  The rule is DESIGN.md 21's, per tensor of the 4 (n_hidden + 1) + 1:
max|g - g64| <= 4 Y max|g64_tensor| + 2^-23 max|g64_model|, Y the float32-vs-float64 torch loss of the case."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import a2c_host as AH
import policy_host as PH
import ppow_host as W
import sacw_host as SWH

ROOT = PH.ROOT
DIR = os.path.join(ROOT, "tests", "hostbuild_a2cw")
ROWS = ((1, 1), (1, 63), (5, 13), (5, 40))
CASES = [(s, T, E) for s in (W.SHAPE_A, W.SHAPE_REF, W.SHAPE_ODD, W.SHAPE_MAX) for T, E in ROWS]
_lib = None
_refs = {}


def sources():
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    return [os.path.join(DIR, "a2cw_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + \
        [os.path.join(csrc, h) for h in ("xarm_a2cw_core.h", "xarm_ppow_core.h", "xarm_sacw_core.h", "xarm_sac_core.h", "xarm_ppo_core.h", "xarm_opt_core.h",
                                         "xarm_a2c_core.h", "xarm_policy_core.h", "xarm_norm_core.h", "xarm_core.h")]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "liba2cw_host.so")
    srcs = sources()
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + SWH.gxx_flags() + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.awh_workspace_bytes.argtypes = [vp]
    L.awh_workspace_bytes.restype = C.c_int64
    L.awh_geometry.argtypes = [vp, vp]
    L.awh_update.argtypes = [vp] * 15
    _lib = L
    return L


def abi_layout(T, E, shape):
    from gym_xarm_amd import _native
    D, A, H, L, act = shape
    return _native.XarmA2CWLayout(E, T, D, A, H, L, W.ACTS[act] if isinstance(act, str) else act)


def geometry(T, E, shape):
    out = np.zeros(48, np.int64)
    lib().awh_geometry(C.byref(abi_layout(T, E, shape)), C.c_void_p(out.ctypes.data))
    nt = int(out[6])
    return {"P": int(out[0]), "N": int(out[1]), "groups": int(out[2]), "head_groups": int(out[3]), "launches": int(out[4]), "ranges": int(out[5]), "NT": nt,
            "blocks": int(out[7]), "rows": [int(v) for v in out[8:25]], "off": [int(v) for v in out[25:25 + nt + 1]],
            "work": dict(zip(("value", "ret", "mean", "hid", "grad"), (int(v) for v in out[43:48])))}


def workspace_floats(T, E, shape):
    """the workspace's size by the helper's own count: each part rounded up to 16 bytes"""
    D, A, H, L, _ = shape
    N = T * E
    P = sum(W.sizes(W.model_of(shape)))
    ptow = P - A
    G = min(64, -(-N // 256))
    ranges = max(1, min(16, -(-N // 64)))
    r4 = lambda n: -(-n // 4) * 4
    parts = [2 * 20, 2 * G * 20, 2 * -(-P // 256), N + E, N, N * A, N * A, N, 2 * L * N * H, 2 * L * N * H, ranges * ptow, P]
    return sum(r4(n) for n in parts)


_p = W._p


def host_update(w, sq, b, h, shape):
    """one update of the host build, in place on the aligned arrays of w and sq; returns (rc, outputs): returns, grad, stats, the workspace,
    the bootstrap values read off it, and the number of launches the chain handed the executor"""
    T, E, _ = b["obs"].shape
    layout, params = abi_layout(T, E, shape), AH.abi_params(h)
    geo = geometry(T, E, shape)
    out = {"returns": np.full((T, E), np.nan, np.float32), "grad": np.full(geo["P"], np.nan, np.float32), "stats": np.full(8, np.nan, np.float32)}
    work = PH.aligned(np.zeros(max(lib().awh_workspace_bytes(C.byref(layout)), 16) // 4, np.float32))
    launched = np.zeros(1, np.int64)
    ws, qs = W.abi_weights(w), W.abi_weights(sq)
    rc = lib().awh_update(C.byref(layout), C.byref(params), C.byref(ws), C.byref(qs), _p(b["obs"]), _p(b["action"]), _p(b["reward"]), _p(b["done"]),
                          _p(b["use"]), _p(b["last_obs"]), _p(work), *[_p(out[k]) for k in ("returns", "grad", "stats")], _p(launched))
    o = geo["work"]["value"] + T * E
    out["boot"] = work[o:o + E].copy()
    out["workspace"] = work
    out["launched"] = int(launched[0])
    return rc, out


def fresh_state(model):
    w = W.weights_of(model)
    return w, W.zeros_like(w)


# ---- torch: train.py's own A2C functions on the batch, in the model's dtype
def torch_grad(model, b, h, dtype):
    """(flat gradient float64 [P] in the update's order, returns [T, E], stats) of a `dtype` copy of the model"""
    m = copy.deepcopy(model).to(dtype)
    loss, rets, st = AH.torch_loss(m, b, h)
    g = np.concatenate([(torch.zeros_like(p) if x is None else x).numpy().astype(np.float64).ravel()
                        for x, p in zip(torch.autograd.grad(loss, W.tensors_of(m), allow_unused=True), W.tensors_of(m))])
    st["grad_norm"] = float(np.sqrt((g * g).sum()))
    return g, rets.numpy(), st


torch_updates = AH.torch_updates            # clip_grad_norm_ + RMSprop.step over the batches on a `dtype` copy of any ActorCritic


def flat_params(model):
    return np.concatenate([t.detach().numpy().astype(np.float64).ravel() for t in W.tensors_of(model)])


def reference(shape, T, E, ent_coef=0.0, masked=True, seed=1):
    """the settled batch, the float64 and float32 torch gradients and the yardstick of one case; computed once and only read"""
    key = (shape, T, E, ent_coef, masked, seed)
    if key not in _refs:
        h = AH.hyper(ent_coef=ent_coef)
        model = W.model_of(shape)
        b, margin, taken = W.settle(model, W.make_batch(shape, T, E, masked, seed))
        g64, ret64, st64 = torch_grad(model, b, h, torch.float64)
        g32, _, _ = torch_grad(model, b, h, torch.float32)
        sz = W.sizes(model)
        _refs[key] = dict(h=h, b=b, g64=g64, g32=g32, ret64=ret64, st64=st64, sizes=sz, margin=margin, taken=taken, Y=W.yardstick(g32, g64, sz))
    return _refs[key]


def check_stats(st, ref, Y, A):
    """stats [8] against the float64 torch terms: a row's loss terms pass through fewer than 8 + 4 A float32 roundings on top of what the
    forward loses (Y's source too); the sums run in float64.  n_use is a sum of zeros and ones; the entropy is A float32 values added in
    float64 (tests/test_a2c_host.py's tolerances)"""
    st = np.asarray(st, np.float64)
    rel = 4.0 * Y + (8 + 4 * A) * 2.0 ** -24
    tol = {"policy_loss": rel * ref["policy_abs"], "value_loss": rel * ref["value_loss"], "entropy": 2.0 ** -23 * max(1.0, abs(ref["entropy"])),
           "grad_norm": rel * ref["grad_norm"], "n_use": 0.0}
    for i, k in enumerate(("policy_loss", "value_loss", "entropy", "grad_norm", "n_use")):
        assert abs(st[i] - ref[k]) <= tol[k] + 2.0 ** -24 * abs(ref[k]), (k, st[i], ref[k], tol[k])
    assert np.all(st[5:] == 0.0)


def parameter_batches(shape, n_updates, h, reward_scale=1.0, T=5, E=13, seed0=0):
    """n_updates batches, each settled (ReLU) under the float64 model that has taken the updates before it, with the float64 / float32 torch
    gradients at that model: [(batch, g64, g32, stats64)]"""
    model = W.model_of(shape)
    out, done = [], []
    for s in range(n_updates):
        m64, _ = torch_updates(model, done, h, torch.float64)
        raw = W.make_batch(shape, T, E, seed=seed0 + s)
        raw["reward"] = (raw["reward"] * np.float32(reward_scale)).astype(np.float32)
        b, _, _ = W.settle(m64, raw)
        g64, _, st = torch_grad(m64, b, h, torch.float64)
        g32, _, _ = torch_grad(m64, b, h, torch.float32)
        out.append((b, g64, g32, st))
        done.append(b)
    return out


def left_out_of(items, sz):
    """bool [P]: entries whose float64 gradient lies within the gradient bound of zero in any of the updates (but is not exactly zero)"""
    left = np.zeros(sum(sz), bool)
    for _, g64, g32, _ in items:
        left |= W.sensitive(g64, W.yardstick(g32, g64, sz), sz)
    return left


def largest_share(left, sz):
    return max(part.sum() / part.size for part in W.split(left, sz))
