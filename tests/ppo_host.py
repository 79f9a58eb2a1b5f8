"""ctypes view of tests/hostbuild_ppo (g++ -ffp-contract=off build of csrc/xarm_ppo_core.h) - CPU-side tests only - with the batches,
the permutations, the test old_logp and the torch reference - train.py's ppo_prepare, ppo_minibatch_loss and optimizer_step on float64 /
float32 copies of the model - that the host and GPU tests share.  Models, rows, the rule and the yardstick come from a2c_host /
policy_host."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import a2c_host as AH
import policy_host as PH
from gym_xarm_amd import train as TR

ROOT = PH.ROOT
DIR = os.path.join(ROOT, "tests", "hostbuild_ppo")
HYPER = ("gamma", "gae_lambda", "clip_range", "lr", "beta1", "beta2", "eps", "vf_coef", "ent_coef", "max_grad_norm")
DEFAULTS = dict(gamma=0.99, gae_lambda=0.95, clip_range=0.2, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5, vf_coef=0.5, ent_coef=0.0, max_grad_norm=0.5,
                normalize_advantage=1)
STATS = ("policy_loss", "value_loss", "entropy", "grad_norm", "n_use", "approx_kl", "clip_fraction")
_lib = None
_refs = {}


def sources():
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    return [os.path.join(DIR, "ppo_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + \
        [os.path.join(csrc, h) for h in ("xarm_ppo_core.h", "xarm_opt_core.h", "xarm_a2c_core.h", "xarm_policy_core.h", "xarm_norm_core.h", "xarm_core.h")]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "libppo_host.so")
    srcs = sources()
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + PH.gxx_flags() + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.ph_workspace_bytes.argtypes = L.ph_param_count.argtypes = [vp]
    L.ph_workspace_bytes.restype = L.ph_param_count.restype = C.c_int64
    L.ph_geometry.argtypes = [vp, vp]
    L.ph_update.argtypes = [vp] * 20
    _lib = L
    return L


def hyper(**kw):
    h = dict(DEFAULTS)
    h.update(kw)
    return h


def abi_params(h):
    from gym_xarm_amd import _native
    return _native.XarmPPOParams(*([float(h[k]) for k in HYPER] + [int(h["normalize_advantage"])]))


def abi_layout(T, E, D, A, n_epochs, batch_size):
    from gym_xarm_amd import _native
    return _native.XarmPPOLayout(E, T, D, A, 64, n_epochs, batch_size)


def geometry(T, E, D, A, n_epochs, batch_size):
    """tiles of a full minibatch, groups, rows per tile, the most groups, rows per minibatch, minibatches, steps, launches"""
    out = np.zeros(8, np.int64)
    lib().ph_geometry(C.byref(abi_layout(T, E, D, A, n_epochs, batch_size)), C.c_void_p(out.ctypes.data))
    return [int(v) for v in out]


def steps_of(N, n_epochs, batch_size):
    B = min(batch_size, N)
    return n_epochs * (-(-N // B))


def make_perm(N, n_epochs, seed=0):
    rs = np.random.RandomState(77 + seed + 3 * N)
    return np.ascontiguousarray(np.stack([rs.permutation(N) for _ in range(n_epochs)]).astype(np.int32))


def make_batch(D, A, T, E, scale, masked=True, seed=1, reward_scale=1.0):
    """a2c_host.make_batch with its standard normal draws taken as the rollout's noise: action = mean + exp(log_std) z under the case's
    model (float64), as a rollout stores it.  Raw standard normal actions lie up to 17 standard deviations from the mean of a policy
    with log_std -1.4 - log-probabilities down to -106, where one float32 unit in the last place is 7.6e-6; a ratio
    exp(logp - old_logp) against a supplied old_logp then carries that rounding (1.8e-6 rms over the rows, host build and torch float32
    alike), and at 16 unclipped rows the gradient's error is a draw of that noise, not a property of the arithmetic under test (5 x 200
    rows, minibatch 64: host build 4.7 Y where torch's own draw was small, the other cases 0.4 - 2.7 Y).
    seed: a2c_host's draw 1 by default.  With draw 0 at 14 x 4, 5 x 13 rows and a supplied old_logp, pi_b3 - the sum of q d iv over the
    20 unclipped of 59 used rows, iv = 17.8 at log_std -1.44 - carries 1.8e-6 of its largest entry in the host build against torch
    float32's 2.8e-7 (3.5 - 5.6 Y) for every draw of old_logp; draws 1 and 2 of the same shape give 0.5 - 1.8 Y."""
    b = AH.make_batch(D, A, T, E, scale, masked, seed, reward_scale)
    m64 = copy.deepcopy(PH.case(D, 0, A, scale)["model"]).to(torch.float64)
    with torch.no_grad():
        mean = m64.pi(_t(b["obs"], torch.float64)).numpy()
        std = m64.log_std.exp().numpy()
    b["action"] = np.ascontiguousarray((mean + std * b["action"].astype(np.float64)).astype(np.float32))
    return b


def host_update(w, m, v, step, b, h, perm, batch_size, old_logp=None):
    """one update of the host build, in place on the aligned arrays of w, m, v and on step (int64 [1]); returns (rc, outputs)"""
    T, E, D = b["obs"].shape
    A = b["action"].shape[2]
    from gym_xarm_amd import _native
    n_epochs = perm.shape[0]
    layout, params = abi_layout(T, E, D, A, n_epochs, batch_size), abi_params(h)
    S = steps_of(T * E, n_epochs, batch_size)
    W = lambda x: _native.XarmPolicyWeights(*[x[k].ctypes.data for k in PH.NAMES])
    ws, ms, vs = W(w), W(m), W(v)
    out = {"adv": np.full((T, E), np.nan, np.float32), "returns": np.full((T, E), np.nan, np.float32), "grad": np.full(sum(AH.sizes(D, A)), np.nan, np.float32),
           "stats": np.full((S, 8), np.nan, np.float32), "old_logp": np.full((T, E), np.nan, np.float32)}
    work = PH.aligned(np.zeros(4, np.float32))
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    rc = lib().ph_update(C.byref(layout), C.byref(params), C.byref(ws), C.byref(ms), C.byref(vs), p(step), p(b["obs"]), p(b["action"]), p(b["reward"]),
                         p(b["done"]), p(b["use"]), p(b["last_obs"]), p(old_logp), p(perm), p(work),
                         *[p(out[k]) for k in ("adv", "returns", "grad", "stats", "old_logp")])
    return rc, out


# ---- torch: train.py's own PPO functions on the batch, in the model's dtype
def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def torch_prepare(model, b, h, old_logp=None):
    """(adv, ret, old_logp, use), flat [N], from the model as it is (no gradient)"""
    dt = model.log_std.dtype
    return TR.ppo_prepare(model, *AH.rollout_of(b, dt), h["gamma"], h["gae_lambda"], None if old_logp is None else _t(old_logp, dt))


def torch_step_loss(model, b, h, prep, idx):
    """the loss of one minibatch (idx: valid rows in position order) and what the tests read of it"""
    loss, t = TR.ppo_minibatch_loss(model, AH.rollout_of(b, model.log_std.dtype)[0], prep, idx, h["clip_range"], h["vf_coef"], h["ent_coef"],
                                    bool(h["normalize_advantage"]), diagnostics=True)
    t = {k: v.detach() for k, v in t.items()}
    st = {k: float(t[k]) for k in ("policy_loss", "value_loss", "entropy", "n_use", "approx_kl", "clip_fraction")}
    st["policy_abs"] = float((t["surr"].abs() * t["use"]).sum() / t["n_use"])
    st["kl_abs"] = float((((t["rho"] - 1.0).abs() + t["log_ratio"].abs()) * t["use"]).sum() / t["n_use"])
    st.update(rho=t["rho"].numpy().astype(np.float64), ahat=t["a_hat"].numpy().astype(np.float64), use=t["use"].numpy().astype(np.float64))
    return loss, st


def step_rows(perm, N, batch_size, s):
    """the valid rows of optimiser step s in position order"""
    B = min(batch_size, N)
    M = -(-N // B)
    ep, m = divmod(s, M)
    idx = perm[ep, m * B:min((m + 1) * B, N)].astype(np.int64)
    return torch.from_numpy(idx[(idx >= 0) & (idx < N)])


def torch_update(model, b, h, perm, batch_size, dtype, old_logp=None, n_steps=None, opt=None):
    """the first n_steps optimiser steps (all by default) on a `dtype` copy: clip_grad_norm_ + Adam.  Returns (model, optimiser, one record
    per step: the flat float64 gradient before the clip, the stats, rho / ahat / use of the step's rows)"""
    m = copy.deepcopy(model).to(dtype)
    N = b["obs"].shape[0] * b["obs"].shape[1]
    if opt is None:
        opt = torch.optim.Adam(m.parameters(), lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
    else:
        opt = opt(m)
    prep = torch_prepare(m, b, h, old_logp)
    S = steps_of(N, perm.shape[0], batch_size)
    recs = []
    for s in range(S if n_steps is None else min(S, n_steps)):
        loss, st = torch_step_loss(m, b, h, prep, step_rows(perm, N, batch_size, s))
        g = np.concatenate([x.numpy().astype(np.float64).ravel() for x in torch.autograd.grad(loss, PH.model_params(m), retain_graph=True)])
        st["grad_norm"] = float(np.sqrt((g * g).sum()))
        st["grad"] = g
        recs.append(st)
        TR.optimizer_step(m, opt, loss, h["max_grad_norm"])
    return m, opt, recs, prep


def assert_valid(recs, h):
    """the condition on a case's inputs: in float64, at every optimiser step, no used row lies within 1e-4 of a clip edge or has
    |A^| < 1e-6 - float32 and float64 then take the same clip branch on every row"""
    eps = h["clip_range"]
    for s, st in enumerate(recs):
        used = st["use"] != 0
        rho, ahat = st["rho"][used], st["ahat"][used]
        if rho.size == 0:
            continue
        edge = np.minimum(np.abs(rho - (1.0 - eps)), np.abs(rho - (1.0 + eps))).min()
        assert edge >= 1e-4 and np.abs(ahat).min() >= 1e-6, "invalid case: step %d has a row at %.2e of a clip edge / |A^| %.2e" % (s, edge, np.abs(ahat).min())


def spread_old_logp(model, b, h, seed=0):
    """the test old_logp [T, E] (float32): the float64 logp minus log rho*, with target ratios rho* drawn so that a third of the rows
    lies below 1 - eps, a third inside and a third above"""
    m64 = copy.deepcopy(model).to(torch.float64)
    T, E = b["reward"].shape
    with torch.no_grad():
        logp = m64.dist(_t(b["obs"], torch.float64)).log_prob(_t(b["action"], torch.float64)).sum(-1).numpy()
    rs = np.random.RandomState(911 + seed + 5 * T * E)
    eps = h["clip_range"]
    kind = rs.permutation(T * E).reshape(T, E) % 3
    lo, hi = np.array([0.5, 1.0 - eps + 0.05, 1.0 + eps + 0.05]), np.array([1.0 - eps - 0.05, 1.0 + eps - 0.05, 1.6])
    rho = rs.uniform(lo[kind], hi[kind])
    return np.ascontiguousarray((logp - np.log(rho)).astype(np.float32))


def reference(D, A, T, E, batch_size, normalize=1, ent_coef=0.0, supplied=True, n_epochs=1, masked=True, scale=1.0, n_steps=1):
    """the batch, perm, old_logp, the float64 / float32 torch records of the first n_steps optimiser steps and step 0's yardstick;
    computed once and only read"""
    key = (D, A, T, E, batch_size, normalize, ent_coef, supplied, n_epochs, masked, scale, n_steps)
    if key not in _refs:
        h = hyper(ent_coef=ent_coef, normalize_advantage=normalize)
        b = make_batch(D, A, T, E, scale, masked)
        model = PH.case(D, 0, A, scale)["model"]
        perm = make_perm(T * E, n_epochs)
        olp = spread_old_logp(model, b, h) if supplied else None
        _, _, r64, prep64 = torch_update(model, b, h, perm, batch_size, torch.float64, olp, n_steps)
        _, _, r32, _ = torch_update(model, b, h, perm, batch_size, torch.float32, olp, n_steps)
        assert_valid(r64, h)
        _refs[key] = dict(h=h, b=b, perm=perm, old_logp=olp, r64=r64, r32=r32, prep64=[x.numpy() for x in prep64],
                          Y=AH.yardstick(r32[0]["grad"], r64[0]["grad"], D, A))
    return _refs[key]


def fresh_state(model):
    """(w, m, v, step) for the host build: the model's weights, zero Adam state"""
    w = PH.weights_of(model)
    return w, AH.zeros_like_weights(w), AH.zeros_like_weights(w), np.zeros(1, np.int64)


# ---- checks shared by the host and the GPU tests
def stat_bounds(ref, Y, A):
    """test_a2c_host.py's bounds for the A2C stats, with approx_kl held like the policy loss: a row's terms pass through fewer than
    8 + 4 A float32 roundings on top of what the forward loses; the sums run in float64.  2^-40 on approx_kl: the float64 reference's own
    rounding of two log-probabilities of size up to 2^6 (with old_logp NULL the device gives exactly 0 and the reference 1e-17)"""
    rel = 4.0 * Y + (8 + 4 * A) * 2.0 ** -24
    return {"policy_loss": rel * ref["policy_abs"], "value_loss": rel * ref["value_loss"], "entropy": 2.0 ** -23 * max(1.0, abs(ref["entropy"])),
            "grad_norm": rel * ref["grad_norm"], "n_use": 0.0, "approx_kl": rel * ref["kl_abs"] + 2.0 ** -40, "clip_fraction": 0.0}


def check_stats(row, ref, Y, A):
    tol = stat_bounds(ref, Y, A)
    for i, k in enumerate(STATS):
        if k == "clip_fraction":               # exact: the same rows are clipped (the validity condition), counted and divided alike
            assert row[i] == np.float32(ref[k]), (k, row[i], ref[k])
        else:
            assert abs(float(row[i]) - ref[k]) <= tol[k] + 2.0 ** -24 * abs(ref[k]), (k, row[i], ref[k], tol[k])
    assert row[7] == 0.0


def parameter_case(D, A, T, E, B, n_epochs, runner):
    """a whole update: float64 and float32 torch, `runner` (the build under test), and the entries left out - those whose float64
    gradient lies within the gradient bound of zero at any of the steps (Adam's first steps are nearly lr sign(g))"""
    r = reference(D, A, T, E, B, 1, 0.0, True, n_epochs=n_epochs, n_steps=1 << 20)
    model = PH.case(D, 0, A, 1.0)["model"]
    m64, _, _, _ = torch_update(model, r["b"], r["h"], r["perm"], B, torch.float64, r["old_logp"])
    m32, _, _, _ = torch_update(model, r["b"], r["h"], r["perm"], B, torch.float32, r["old_logp"])
    left_out = np.zeros(sum(AH.sizes(D, A)), bool)
    for s64, s32 in zip(r["r64"], r["r32"]):
        left_out |= AH.sensitive(s64["grad"], AH.yardstick(s32["grad"], s64["grad"], D, A), D, A)
    for part in AH.split(left_out, D, A):
        assert part.sum() <= 0.01 * part.size, "more than 1 % of a tensor's entries have a float64 gradient at zero"
    p = runner(r)
    p64 = np.concatenate([x.detach().numpy().ravel() for x in PH.model_params(m64)])
    p32 = AH.flat_of(PH.weights_of(m32))
    keep = ~left_out
    Y = AH.yardstick(np.where(keep, p32, p64), p64, D, A)
    ratio, in_y = AH.rule(p, p64, Y, D, A, keep)
    assert np.abs(p - AH.flat_of(PH.weights_of(model))).max() > 1e-4                    # the update moved the parameters
    return ratio, in_y, Y, int(left_out.sum()), len(r["r64"])


def out_of_range_pair(D, A, T, E):
    """(batch, perm of one epoch with a tenth of its entries replaced by -1 and N, the batch with those rows' use zeroed, the clean
    perm): the two calls that must agree bit for bit"""
    N = T * E
    b = make_batch(D, A, T, E, 1.0)
    perm = make_perm(N, 1)
    bad = perm.copy()
    pos = np.random.RandomState(5).permutation(N)[:max(N // 10, 2)]
    bad[0, pos[0::2]] = -1
    bad[0, pos[1::2]] = N
    b0 = dict(b, use=b["use"].copy())
    b0["use"].reshape(-1)[perm[0, pos]] = 0.0
    return b, bad, b0, perm
