"""ctypes view of tests/hostbuild_ppow (g++ -ffp-contract=off build of csrc/xarm_acw_core.h and csrc/xarm_ppow_core.h) - CPU-side tests
only - with the models, batches and the torch reference that the host and GPU tests of the wide MlpPolicy and the wide PPO update share.
The reference is train.py's own ppo_prepare / ppo_minibatch_loss / optimizer_step on float64 and float32 copies of the same
ActorCritic(net_arch, activation), reached through ppo_host's helpers; the rule is DESIGN.md 21's, per tensor of the 4 (n_hidden + 1) + 1:
max|g - g64| <= 4 Y max|g64_tensor| + 2^-23 max|g64_model|, Y the float32-vs-float64 torch loss of the case.

Validity: ppo_host.assert_valid (no used row within 1e-4 of a clip edge or with |A^| < 1e-6 in float64) and, for ReLU, DESIGN.md 24's
condition - a used row's hidden pre-activations of both towers lie at least m from 0 in float64, m = 4 x the deviation of float32 from
float64 taken with both precisions on the SAME parameters (the float64 model rounded to float32).  `settle` takes the rows inside out
through `use`; a case may lose at most 20 % of its rows that way (asserted)."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import a2c_host as AH
import policy_host as PH
import ppo_host as PP
import sacw_host as SWH
from gym_xarm_amd import train as TR

ROOT = PH.ROOT
DIR = os.path.join(ROOT, "tests", "hostbuild_ppow")
ACTS = {"tanh": 0, "relu": 1}
# (D, A, hidden, n_hidden, activation)
SHAPE_A, SHAPE_REF = (14, 4, 128, 2, "relu"), (30, 4, 256, 3, "relu")
SHAPE_ODD, SHAPE_MAX, SHAPE_CROSS = (29, 1, 192, 3, "tanh"), (96, 16, 256, 2, "tanh"), (14, 4, 64, 2, "tanh")
BASE = [(s, T, E) for s in (SHAPE_A, SHAPE_REF) for T, E in ((1, 1), (1, 63), (5, 13), (5, 40))]
CASES = BASE + [(SHAPE_ODD, 5, 13), (SHAPE_MAX, 5, 13)]
BATCH = 33                                  # two minibatches at 5 x 13 with a short last one
_lib = None
_models, _refs = {}, {}


def case_id(c):
    (D, A, H, L, act), T, E = c
    return "D%d-A%d-%dx%d-%s-%dx%d" % (D, A, H, L, act, T, E)


def sources():
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    return [os.path.join(DIR, "ppow_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + \
        [os.path.join(csrc, h) for h in ("xarm_ppow_core.h", "xarm_acw_core.h", "xarm_sacw_core.h", "xarm_sac_core.h", "xarm_ppo_core.h", "xarm_opt_core.h",
                                         "xarm_a2c_core.h", "xarm_policy_core.h", "xarm_norm_core.h", "xarm_core.h")]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "libppow_host.so")
    srcs = sources()
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + SWH.gxx_flags() + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.pwh_workspace_bytes.argtypes = L.pwh_act_workspace_bytes.argtypes = [vp]
    L.pwh_workspace_bytes.restype = L.pwh_act_workspace_bytes.restype = C.c_int64
    L.pwh_geometry.argtypes = [vp, vp]
    L.pwh_act.argtypes = [vp] * 13
    L.pwh_update.argtypes = [vp] * 19
    _lib = L
    return L


# ---- models and their tensors
def model_of(shape):
    """a private copy of the case's ActorCritic: torch's default initialisation under a seed of the shape, log_std drawn in [-1.2, -0.3]"""
    if shape not in _models:
        D, A, H, L, act = shape
        gen = torch.random.get_rng_state()
        torch.manual_seed(1000 + 7 * D + A + 3 * H + L + (500 if act == "relu" else 0))
        m = TR.ActorCritic(D, A, (H,) * L, act)
        with torch.no_grad():
            m.log_std.copy_(torch.from_numpy(np.random.RandomState(D + A).uniform(-1.2, -0.3, A).astype(np.float32)))
        torch.random.set_rng_state(gen)
        _models[shape] = m
    return copy.deepcopy(_models[shape])


def tensors_of(model):
    """pi's tensors, vf's, log_std: the flat order of the update"""
    from gym_xarm_amd.device_policy import tower_params
    pi, vf = tower_params(model)
    return list(pi) + list(vf) + [model.log_std]


def sizes(model):
    return [int(t.numel()) for t in tensors_of(model)]


def weights_of(model):
    return [PH.aligned(t.detach().cpu().numpy()) for t in tensors_of(model)]


def zeros_like(w):
    return [PH.aligned(np.zeros_like(a)) for a in w]


def flat_of(w):
    return np.concatenate([np.asarray(a, np.float64).ravel() for a in w])


def split(flat, sz):
    o = np.cumsum([0] + list(sz))
    return [flat[o[i]:o[i + 1]] for i in range(len(sz))]


def abi_weights(ws):
    """an xarm_acw_weights over aligned arrays in the flat order (None entries stay NULL)"""
    from gym_xarm_amd import _native
    tp = (len(ws) - 1) // 2
    s = _native.XarmACWWeights()
    for i, a in enumerate(ws[:-1]):
        if a is not None:
            (s.pi if i < tp else s.vf)[i % tp] = a.ctypes.data
    if ws[-1] is not None:
        s.log_std = ws[-1].ctypes.data
    return s


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


# ---- the act call
def act_layout(rows, shape, goal_dim=0, row_offset=0):
    from gym_xarm_amd import _native
    D, A, H, L, act = shape
    return _native.XarmACWLayout(rows, D - 2 * goal_dim, goal_dim, A, H, L, ACTS[act] if isinstance(act, str) else act, row_offset)


def host_act(w, rows, shape, goal_dim=0, stats=None, deterministic=False, seed=0, row_offset=0, calls=None, value=True, clip_obs=10.0, eps=1e-8):
    """one act call of the host build on the rows [E, D]; returns the four outputs (filled with NaN first) and the workspace"""
    from gym_xarm_amd import _native
    E, A = rows.shape[0], shape[1]
    layout = act_layout(E, shape, goal_dim, row_offset)
    params = _native.XarmPolicyParams(seed, clip_obs, eps, int(deterministic))
    calls = np.zeros(1, np.int64) if calls is None else calls
    out = {"action": np.full((E, A), np.nan, np.float32), "env_action": np.full((E, A), np.nan, np.float32), "logp": np.full(E, np.nan, np.float32),
           "value": np.full(E, np.nan, np.float32) if value else None}
    work = PH.aligned(np.zeros(max(lib().pwh_act_workspace_bytes(C.byref(layout)), 16) // 4, np.float32))
    parts = PH.split(rows, shape[0] - 2 * goal_dim, goal_dim)
    ws = abi_weights(w)
    rc = lib().pwh_act(C.byref(layout), C.byref(params), C.byref(ws), _p(stats), _p(calls), *[_p(x) for x in parts], _p(work),
                       *[_p(out[k]) for k in ("action", "env_action", "logp", "value")])
    assert rc == 0
    out["workspace"] = work
    return out


# ---- the update
def abi_layout(T, E, shape, n_epochs, batch_size):
    from gym_xarm_amd import _native
    D, A, H, L, act = shape
    return _native.XarmPPOWLayout(E, T, D, A, H, L, ACTS[act] if isinstance(act, str) else act, n_epochs, batch_size)


def geometry(T, E, shape, n_epochs, batch_size):
    out = np.zeros(48, np.int64)
    lib().pwh_geometry(C.byref(abi_layout(T, E, shape, n_epochs, batch_size)), C.c_void_p(out.ctypes.data))
    nt = int(out[7])
    return {"P": int(out[0]), "B": int(out[1]), "M": int(out[2]), "S": int(out[3]), "chunks": int(out[4]), "launches": int(out[5]), "ranges": int(out[6]),
            "NT": nt, "rows": [int(v) for v in out[8:25]], "off": [int(v) for v in out[25:25 + nt + 1]],
            "work": dict(zip(("mean", "value", "adv", "ret", "old_logp"), (int(v) for v in out[43:48])))}


def make_batch(shape, T, E, masked=True, seed=1):
    """rows uniform in [-2.5, 2.5], stored actions mean + exp(log_std) z under the case's model in float64 (what a rollout stores), standard
    normal rewards, 10 % episode ends, a use mask with about 10 % zeros"""
    D, A = shape[:2]
    N = T * E
    rs = np.random.RandomState(1000 * seed + 7 * D + A + 131 * N + shape[2])
    rows = rs.uniform(-2.5, 2.5, (N + E, D)).astype(np.float32)
    z = rs.standard_normal((T, E, A))
    b = {"obs": np.ascontiguousarray(rows[:N].reshape(T, E, D)), "last_obs": np.ascontiguousarray(rows[N:]),
         "reward": rs.standard_normal((T, E)).astype(np.float32), "done": (rs.uniform(size=(T, E)) < 0.1).astype(np.float32),
         "use": (rs.uniform(size=(T, E)) >= 0.1).astype(np.float32) if masked else None}
    m64 = model_of(shape).to(torch.float64)
    with torch.no_grad():
        mean = m64.pi(torch.from_numpy(b["obs"]).double()).numpy()
        std = m64.log_std.exp().numpy()
    b["action"] = np.ascontiguousarray((mean + std * z).astype(np.float32))
    return b


def host_update(w, m, v, step, b, h, perm, batch_size, shape, old_logp=None):
    """one update of the host build, in place on the aligned arrays of w, m, v and on step (int64 [1]); returns (rc, outputs): adv,
    returns, grad, stats, old_logp (read off the workspace) and the workspace itself"""
    T, E, _ = b["obs"].shape
    n_epochs = perm.shape[0]
    layout, params = abi_layout(T, E, shape, n_epochs, batch_size), PP.abi_params(h)
    geo = geometry(T, E, shape, n_epochs, batch_size)
    out = {"adv": np.full((T, E), np.nan, np.float32), "returns": np.full((T, E), np.nan, np.float32), "grad": np.full(geo["P"], np.nan, np.float32),
           "stats": np.full((max(geo["S"], 1), 8), np.nan, np.float32)}
    work = PH.aligned(np.zeros(max(lib().pwh_workspace_bytes(C.byref(layout)), 16) // 4, np.float32))
    ws, ms, vs = abi_weights(w), abi_weights(m), abi_weights(v)
    rc = lib().pwh_update(C.byref(layout), C.byref(params), C.byref(ws), C.byref(ms), C.byref(vs), _p(step), _p(b["obs"]), _p(b["action"]), _p(b["reward"]),
                          _p(b["done"]), _p(b["use"]), _p(b["last_obs"]), _p(old_logp), _p(perm), _p(work),
                          *[_p(out[k]) for k in ("adv", "returns", "grad", "stats")])
    o = geo["work"]["old_logp"]
    out["old_logp"] = old_logp if old_logp is not None else work[o:o + T * E].reshape(T, E).copy()
    out["workspace"] = work
    return rc, out


def fresh_state(model):
    w = weights_of(model)
    return w, zeros_like(w), zeros_like(w), np.zeros(1, np.int64)


# ---- torch: train.py's own PPO functions on the batch, in the model's dtype
def torch_update(model, b, h, perm, batch_size, dtype, old_logp=None, n_steps=None):
    """ppo_host.torch_update for any shape: the first n_steps optimiser steps (all by default) on a `dtype` copy.  Returns (model, optimiser,
    one record per step - the flat float64 gradient before the clip, the stats, rho / ahat / use of the step's rows - and the prep)"""
    m = copy.deepcopy(model).to(dtype)
    N = b["obs"].shape[0] * b["obs"].shape[1]
    opt = torch.optim.Adam(m.parameters(), lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
    prep = PP.torch_prepare(m, b, h, old_logp)
    S = PP.steps_of(N, perm.shape[0], batch_size)
    recs = []
    for s in range(S if n_steps is None else min(S, n_steps)):
        loss, st = PP.torch_step_loss(m, b, h, prep, PP.step_rows(perm, N, batch_size, s))
        g = np.concatenate([x.numpy().astype(np.float64).ravel() for x in torch.autograd.grad(loss, tensors_of(m), retain_graph=True, allow_unused=True)])
        st["grad_norm"] = float(np.sqrt((g * g).sum()))
        st["grad"] = g
        recs.append(st)
        TR.optimizer_step(m, opt, loss, h["max_grad_norm"])
    return m, opt, recs, prep


def preacts(model, x):
    """the hidden pre-activations of both towers on the rows x, [rows, 2 n_hidden hidden]"""
    out = []
    with torch.no_grad():
        for tower in (model.pi, model.vf):
            h = x
            for layer in list(tower)[:-1]:
                h = layer(h)
                if isinstance(layer, torch.nn.Linear):
                    out.append(h)
    return torch.cat(out, dim=-1)


def settle(model, b):
    """for ReLU: (the batch with the rows inside the margin taken out through use, m, rows taken out); the margin is 4 x the deviation of
    the float32 pre-activations from float64's with both on the same parameters"""
    if getattr(model, "activation", "tanh") != "relu":
        return b, 0.0, 0
    T, E, D = b["obs"].shape
    m64 = copy.deepcopy(model).to(torch.float64)
    m32 = copy.deepcopy(m64).to(torch.float32)
    x = torch.from_numpy(b["obs"].reshape(T * E, D))
    p64 = preacts(m64, x.double()).numpy()
    p32 = preacts(m32, x).numpy().astype(np.float64)
    margin = 4.0 * np.abs(p32 - p64).max()
    inside = (np.abs(p64) < margin).any(axis=1).reshape(T, E)
    use = np.ones((T, E), np.float32) if b["use"] is None else b["use"].copy()
    taken = int((inside & (use != 0)).sum())
    assert taken <= 0.2 * T * E, "the ReLU margin %.2e takes %d of %d rows: over the 20 %% cap" % (margin, taken, T * E)
    use[inside] = 0.0
    return dict(b, use=use), float(margin), taken


# ---- the rule
def yardstick(x32, x64, sz):
    y = 0.0
    for a, r in zip(split(np.asarray(x32, np.float64), sz), split(x64, sz)):
        m = np.abs(r).max()
        if m > 0.0:
            y = max(y, np.abs(a - r).max() / m)
    return y


def bounds(x64, Y, sz):
    floor = 2.0 ** -23 * np.abs(x64).max()
    return [4.0 * Y * np.abs(r).max() + floor for r in split(x64, sz)]


def rule(x, x64, Y, sz, keep=None):
    """(worst error / bound over the tensors, worst error relative to the tensor's largest entry in units of Y)"""
    worst, in_y = 0.0, 0.0
    keep = np.ones(x64.shape, bool) if keep is None else keep
    for a, r, k, bd in zip(split(np.asarray(x, np.float64), sz), split(x64, sz), split(keep, sz), bounds(x64, Y, sz)):
        if not k.any():
            continue
        err = np.abs(a - r)[k].max()
        worst = max(worst, err / bd if bd > 0 else (0.0 if err == 0 else np.inf))
        if np.abs(r).max() > 0 and Y > 0:
            in_y = max(in_y, err / np.abs(r).max() / Y)
    return worst, in_y


def sensitive(g64, Y, sz):
    """bool [P]: gradient entries within the gradient rule's bound of zero - Adam's first steps are nearly lr sign(g), so their parameters
    are left out of the parameter comparison - but not exactly zero (sacw_host.parameter_case: a ReLU unit that is off on every used row
    by at least the margin is zero in float32 too, and Adam leaves its weights alone)"""
    return np.concatenate([(np.abs(r) <= bd) & (r != 0.0) for r, bd in zip(split(g64, sz), bounds(g64, Y, sz))])


def reference(shape, T, E, batch_size=BATCH, normalize=1, ent_coef=0.0, supplied=True, n_epochs=1, masked=True, n_steps=1):
    """the settled batch, perm, old_logp, the float64 / float32 torch records of the first n_steps optimiser steps and step 0's yardstick;
    computed once and only read"""
    key = (shape, T, E, batch_size, normalize, ent_coef, supplied, n_epochs, masked, n_steps)
    if key not in _refs:
        h = PP.hyper(ent_coef=ent_coef, normalize_advantage=normalize)
        model = model_of(shape)
        b, margin, taken = settle(model, make_batch(shape, T, E, masked))
        perm = PP.make_perm(T * E, n_epochs)
        olp = PP.spread_old_logp(model, b, h) if supplied else None
        _, _, r64, prep64 = torch_update(model, b, h, perm, batch_size, torch.float64, olp, n_steps)
        _, _, r32, _ = torch_update(model, b, h, perm, batch_size, torch.float32, olp, n_steps)
        PP.assert_valid(r64, h)
        sz = sizes(model)
        _refs[key] = dict(h=h, b=b, perm=perm, old_logp=olp, r64=r64, r32=r32, prep64=[x.numpy() for x in prep64], sizes=sz, margin=margin, taken=taken,
                          Y=yardstick(r32[0]["grad"], r64[0]["grad"], sz))
    return _refs[key]
