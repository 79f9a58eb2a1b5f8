"""What the tests of the PPO options (clip_range_vf, target_kl: include/xarm_hip.h xarm_ppo_options) share: the ctypes view of
tests/hostbuild_ppo_opt - the g++ -ffp-contract=off build of csrc/xarm_ppo_core.h and csrc/xarm_ppow_core.h with the options passed
through - and the torch reference, train.py's own ppo_prepare / ppo_old_values / ppo_minibatch_loss / optimizer_step on float64 and
float32 copies of the model with the same two options.  Models, batches, perms, the rule and the stats' bounds are ppo_host's,
ppow_host's, a2c_host's and policy_host's.

A case is (kind, D, A, T, E, B, n_epochs[, hidden, n_hidden, activation]): kind "tile" is the fused 64-row tile's core on
policy_host's 64-64 tanh model and ppo_host's batch, kind "wide" the GEMM chain's core on ppow_host's model and (settled) batch."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import a2c_host as AH
import policy_host as PH
import ppo_host as PP
import ppow_host as W
import sacw_host as SWH
from gym_xarm_amd import train as TR

ROOT = PH.ROOT
DIR = os.path.join(ROOT, "tests", "hostbuild_ppo_opt")
ROWS = ((14, 4, 5, 13, 20, 3), (30, 4, 3, 40, 32, 2))          # D, A, T, E, B, n_epochs: 65 rows in 12 steps (last minibatch 5), 120 in 8 (24)
TILE = [("tile",) + r for r in ROWS]
WIDE = [("wide",) + r + arch for r in ROWS for arch in ((64, 2, "tanh"), (256, 3, "relu"))]
LR = 1e-3
# per case, chosen on the float64 torch reference alone (the tests assert the conditions on it, assert_valid_clip / assert_valid_stop):
# clip_range_vf with every used row at least 1e-4 from the clip's edge and 31 - 46 % of the row-steps clipped; target_kl whose 1.5-fold
# falls into a gap of the float64 approx_kl series (old_logp computed at call start) - "mid" inside an epoch, "epoch" on the first step
# of an epoch
SETTINGS = {TILE[0]: dict(c_vf=0.1, mid=0.02, epoch=0.04), TILE[1]: dict(c_vf=0.08, mid=0.02, epoch=0.05),
            WIDE[0]: dict(c_vf=0.1, mid=0.02, epoch=0.033), WIDE[1]: dict(c_vf=0.15, mid=0.02, epoch=0.2),
            WIDE[2]: dict(c_vf=0.07, mid=0.01, epoch=0.02), WIDE[3]: dict(c_vf=0.25, mid=0.02, epoch=0.13, seed=4)}
# seed: ppow_host.make_batch's draw (1 unless named).  At [256, 256, 256] ReLU and 120 rows draw 1 leaves 1.7 % of a 1024-entry tensor out of
# the parameter rule over the 8 steps in float64 (the cap is 1 %); draw 4 leaves 0.70 %
_lib = None
_cache = {}


def case_id(c):
    return "-".join(str(x) for x in c)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "libppo_opt_host.so")
    srcs = [os.path.join(DIR, "ppo_opt_host.cpp")] + PP.sources()[1:] + W.sources()[1:]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + SWH.gxx_flags() + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    L.poh_update.argtypes = [C.c_void_p] * 20 + [C.c_int64, C.c_void_p]
    L.powh_update.argtypes = [C.c_void_p] * 20 + [C.c_int64]
    L.powh_workspace_bytes.argtypes = [C.c_void_p]
    L.powh_workspace_bytes.restype = C.c_int64
    _lib = L
    return L


def options(clip_range_vf=None, target_kl=None):
    """an xarm_ppo_options, or None (NULL) when both are None"""
    from gym_xarm_amd import _native
    if clip_range_vf is None and target_kl is None:
        return None
    return _native.XarmPPOOptions(float(clip_range_vf or 0.0), float(target_kl or 0.0))


# ---- a case's model, batch, perm
def shape_of(c):
    return (c[1], c[2]) + tuple(c[7:10])


def model_of(c):
    return AH.model_of(c[1], c[2], 1.0) if c[0] == "tile" else W.model_of(shape_of(c))


def tensors_of(c, model):
    return list(PH.model_params(model)) if c[0] == "tile" else W.tensors_of(model)


def sizes_of(c):
    return [int(t.numel()) for t in tensors_of(c, model_of(c))]


def batch_of(c):
    """the suite's masked batch of the case's rows (for "wide": settled, so that ReLU rows at the margin are out through use)"""
    key = ("batch", c)
    if key not in _cache:
        kind, D, A, T, E = c[:5]
        _cache[key] = PP.make_batch(D, A, T, E, 1.0) if kind == "tile" else W.settle(model_of(c), W.make_batch(shape_of(c), T, E, seed=SETTINGS[c].get("seed", 1)))[0]
    return _cache[key]


def perm_of(c, n_epochs=None):
    return PP.make_perm(c[3] * c[4], c[6] if n_epochs is None else n_epochs)


def steps_of(c):
    return PP.steps_of(c[3] * c[4], c[6], c[5])


def fresh_state(c, model=None):
    model = model_of(c) if model is None else model
    return PP.fresh_state(model) if c[0] == "tile" else W.fresh_state(model)


def state_arrays(c, state):
    """the arrays of (w, m, v, step) in one list: what a bit-for-bit comparison walks"""
    w, m, v, step = state
    part = (lambda x: [x[k] for k in PH.NAMES]) if c[0] == "tile" else list
    return part(w) + part(m) + part(v) + [step]


def flat_of(c, w):
    return AH.flat_of(w) if c[0] == "tile" else W.flat_of(w)


def same_bits(xs, ys):
    return all(np.asarray(x).shape == np.asarray(y).shape and PH.bits(np.asarray(x)) == PH.bits(np.asarray(y)) for x, y in zip(xs, ys))


# ---- the host builds
def host_update(c, state, h, perm, old_logp=None, opts=None, b=None, max_steps=-1):
    """one update of the case's host build with the options `opts` (an xarm_ppo_options or None), in place on state = (w, m, v, step);
    returns (rc, {"adv", "returns", "grad", "stats"}).  max_steps >= 0: the call ends after that many optimiser steps"""
    from gym_xarm_amd import _native
    kind, D, A, T, E, B = c[:6]
    b = batch_of(c) if b is None else b
    w, m, v, step = state
    S = PP.steps_of(T * E, perm.shape[0], B)
    out = {"adv": np.full((T, E), np.nan, np.float32), "returns": np.full((T, E), np.nan, np.float32), "grad": np.full(sum(sizes_of(c)), np.nan, np.float32),
           "stats": np.full((S, 8), np.nan, np.float32)}
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    data = [p(step), p(b["obs"]), p(b["action"]), p(b["reward"]), p(b["done"]), p(b["use"]), p(b["last_obs"]), p(old_logp), p(perm)]
    outs = [p(out[k]) for k in ("adv", "returns", "grad", "stats")]
    o = None if opts is None else C.byref(opts)
    if kind == "tile":
        layout = PP.abi_layout(T, E, D, A, perm.shape[0], B)
        S3 = [_native.XarmPolicyWeights(*[x[k].ctypes.data for k in PH.NAMES]) for x in (w, m, v)]
        work = PH.aligned(np.zeros(4, np.float32))
        rc = lib().poh_update(C.byref(layout), C.byref(PP.abi_params(h)), *[C.byref(s) for s in S3], *data, p(work), *outs, o, max_steps, None)
    else:
        layout = W.abi_layout(T, E, shape_of(c), perm.shape[0], B)
        S3 = [W.abi_weights(x) for x in (w, m, v)]
        work = PH.aligned(np.zeros(max(lib().powh_workspace_bytes(C.byref(layout)), 16) // 4, np.float32))
        rc = lib().powh_update(C.byref(layout), C.byref(PP.abi_params(h)), *[C.byref(s) for s in S3], *data, p(work), *outs, o, max_steps)
    return rc, out


# ---- torch with the options
def torch_run(c, h, perm, dtype, old_logp=None, clip_range_vf=None, target_kl=None, b=None):
    """train.py's PPO block on a `dtype` copy of the case's model, minibatches through `perm` as the device takes them.  Returns
    {"model", "recs", "stop"}: one record per step that was reached - ppo_host.torch_step_loss's entries, the flat float64 gradient, and
    the used rows' value under the step's weights `v` and at call start `v0` - and the step whose approx_kl exceeded 1.5 target_kl
    (None: the update ran through); that step's record is there, its optimiser step is not taken"""
    b = batch_of(c) if b is None else b
    m = copy.deepcopy(model_of(c)).to(dtype)
    N, B = c[3] * c[4], c[5]
    opt = torch.optim.Adam(m.parameters(), lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
    rollout = AH.rollout_of(b, dtype)[0]
    prep = PP.torch_prepare(m, b, h, old_logp)
    v0 = TR.ppo_old_values(m, rollout)
    recs, stop = [], None
    for s in range(PP.steps_of(N, perm.shape[0], B)):
        idx = PP.step_rows(perm, N, B, s)
        loss, t = TR.ppo_minibatch_loss(m, rollout, prep, idx, h["clip_range"], h["vf_coef"], h["ent_coef"], bool(h["normalize_advantage"]), diagnostics=True,
                                        clip_range_vf=clip_range_vf, old_values=v0 if clip_range_vf is not None else None)
        t = {k: x.detach() for k, x in t.items()}
        st = {k: float(t[k]) for k in ("policy_loss", "value_loss", "entropy", "n_use", "approx_kl", "clip_fraction")}
        st["policy_abs"] = float((t["surr"].abs() * t["use"]).sum() / t["n_use"])
        st["kl_abs"] = float((((t["rho"] - 1.0).abs() + t["log_ratio"].abs()) * t["use"]).sum() / t["n_use"])
        st.update(rho=t["rho"].numpy().astype(np.float64), ahat=t["a_hat"].numpy().astype(np.float64), use=t["use"].numpy().astype(np.float64),
                  v=t["value"].numpy().astype(np.float64), v0=v0[idx].numpy().astype(np.float64))
        g = np.concatenate([(torch.zeros_like(p) if x is None else x).numpy().astype(np.float64).ravel()
                            for p, x in zip(tensors_of(c, m), torch.autograd.grad(loss, tensors_of(c, m), retain_graph=True, allow_unused=True))])
        st["grad_norm"], st["grad"] = float(np.sqrt((g * g).sum())), g
        recs.append(st)
        if target_kl is not None and st["approx_kl"] > 1.5 * target_kl:
            stop = s
            break
        TR.optimizer_step(m, opt, loss, h["max_grad_norm"])
    return {"model": m, "recs": recs, "stop": stop}


def reference(c, old_logp="spread", clip_range_vf=None, target_kl=None, lr=LR):
    """the case's hyper-parameters, perm, old_logp ("spread": ppo_host.spread_old_logp; None: computed at call start) and the float64 and
    float32 torch runs with the options; computed once and only read"""
    key = ("ref", c, old_logp, clip_range_vf, target_kl, lr)
    if key not in _cache:
        h = PP.hyper(lr=lr)
        perm = perm_of(c)
        olp = PP.spread_old_logp(model_of(c), batch_of(c), h) if old_logp == "spread" else None
        r64 = torch_run(c, h, perm, torch.float64, olp, clip_range_vf, target_kl)
        r32 = torch_run(c, h, perm, torch.float32, olp, clip_range_vf, target_kl)
        _cache[key] = dict(h=h, perm=perm, old_logp=olp, r64=r64, r32=r32, sizes=sizes_of(c))
    return _cache[key]


# ---- validity of a case, asserted on the float64 reference
def clip_shares(recs, c_vf):
    """(smallest distance of a used row's |v - v0| from c_vf over all steps, share of the used row-steps behind step 0 that are clipped)"""
    edge, clipped, used = np.inf, 0, 0
    for s, st in enumerate(recs):
        u = st["use"] != 0
        if not u.any():
            continue
        d = np.abs(st["v"][u] - st["v0"][u])
        edge = min(edge, np.abs(d - c_vf).min())
        if s > 0:
            clipped += int((d > c_vf).sum())
            used += int(u.sum())
    return edge, clipped / max(used, 1)


def assert_valid_clip(recs, h, c_vf):
    """ppo_host.assert_valid (ratio and A^ away from their edges) and the value clip's own condition: no used row within 1e-4 of the
    clip edge at any step, and between a quarter and three quarters of the used row-steps behind step 0 clipped"""
    PP.assert_valid(recs, h)
    edge, share = clip_shares(recs, c_vf)
    assert edge >= 1e-4, "invalid case: a used row lies %.2e from the value clip's edge" % edge
    assert 0.25 <= share <= 0.75, "invalid case: %.1f %% of the used row-steps are clipped" % (100 * share)


def assert_valid_stop(r, target_kl, A):
    """the KL stop's condition on the float64 run of reference `r`: it trips, every approx_kl before s* lies below 1.5 target_kl and the
    one at s* above it, by at least 100 x ppo_host.stat_bounds' bound for approx_kl under the step's own yardstick (float32 and float64
    then take the same decision at every step).  Returns s*"""
    recs, s_star, sz = r["r64"]["recs"], r["r64"]["stop"], r["sizes"]
    assert s_star is not None and len(recs) == s_star + 1 and len(r["r32"]["recs"]) >= s_star + 1
    for s, st in enumerate(recs):
        Y = W.yardstick(r["r32"]["recs"][s]["grad"], st["grad"], sz)
        margin = 100.0 * PP.stat_bounds(st, Y, A)["approx_kl"]
        gap = st["approx_kl"] - 1.5 * target_kl
        assert (gap >= margin) if s == s_star else (gap <= -margin), \
            "invalid case: approx_kl %.3e at step %d lies %.1e from 1.5 target_kl (margin %.1e)" % (st["approx_kl"], s, gap, margin)
    return s_star


# ---- the rule and the stats
def sensitive(c, g64, Y, sz):
    """the entries the parameter rule leaves out: ppo_host.parameter_case's for "tile", ppow_host.sensitive for "wide" (a ReLU unit that is
    off on every used row has a gradient of exactly zero in float32 too and stays in)"""
    if c[0] == "wide":
        return W.sensitive(g64, Y, sz)
    return np.concatenate([np.abs(r) <= bd for r, bd in zip(W.split(g64, sz), W.bounds(g64, Y, sz))])


def parameter_rule(c, r, p):
    """ppo_host.parameter_case's rule for the flat parameters `p` of the build under test against the float64 run of reference `r`:
    (error / bound, error in Y, Y, entries left out).  Left out: entries whose float64 gradient lies within the gradient bound of zero at
    any applied step, at most 1 % of a tensor"""
    sz = r["sizes"]
    applied = len(r["r64"]["recs"]) - (0 if r["r64"]["stop"] is None else 1)
    left_out = np.zeros(sum(sz), bool)
    for s64, s32 in list(zip(r["r64"]["recs"], r["r32"]["recs"]))[:applied]:
        left_out |= sensitive(c, s64["grad"], W.yardstick(s32["grad"], s64["grad"], sz), sz)
    for part in W.split(left_out, sz):
        assert part.sum() <= 0.01 * part.size, "more than 1 % of a tensor's entries have a float64 gradient at zero"
    p64 = np.concatenate([t.detach().numpy().astype(np.float64).ravel() for t in tensors_of(c, r["r64"]["model"])])
    p32 = np.concatenate([t.detach().numpy().astype(np.float64).ravel() for t in tensors_of(c, r["r32"]["model"])])
    keep = ~left_out
    Y = W.yardstick(np.where(keep, p32, p64), p64, sz)
    ratio, in_y = W.rule(p, p64, Y, sz, keep)
    return ratio, in_y, Y, int(left_out.sum())


def check_rows(c, r, stats):
    """every stats row of an update against the float64 run: ppo_host.check_stats's bounds with the step's own yardstick for the applied
    rows; the tripping row the same but grad_norm 0 and column 7 equal to 1; rows behind it zero but for column 7"""
    A, sz = c[2], r["sizes"]
    recs, stop = r["r64"]["recs"], r["r64"]["stop"]
    for s, row in enumerate(stats):
        if stop is not None and s > stop:
            assert np.array_equal(row, np.array([0, 0, 0, 0, 0, 0, 0, 1], np.float32)), (s, row)
            continue
        Y = W.yardstick(r["r32"]["recs"][s]["grad"], recs[s]["grad"], sz)
        if s == stop:
            assert row[3] == 0.0 and row[7] == 1.0, (s, row)
            PP.check_stats(np.concatenate([row[:3], [np.float32(recs[s]["grad_norm"])], row[4:7], [np.float32(0)]]), recs[s], Y, A)
        else:
            PP.check_stats(row, recs[s], Y, A)
