"""ctypes view of tests/hostbuild_sacw (g++ -ffp-contract=off build of csrc/xarm_sacw_core.h) - CPU-side tests only - with the models,
the cases, the torch restatement (sac_host.torch_step on a float64 / float32 copy of the same SacPolicy(net_arch, activation), fed the
same z) and sac_host's tolerance rule generalised to 2 (n_hidden + 1) tensors per tower: per tensor
max|g - g64| <= 4 Y max|g64_tensor| + 2^-23 max|g64_group|, the groups the three optimisers', Y the largest relative loss of torch's
float32 autograd against float64 over the case's trained tensors.

Validity: sac_host's two conditions (no q1 / q2 tie at the actor step, no log_std at a clamp edge) and, for ReLU, a third - the
derivative jumps at 0, so a used row must have, in float64, every hidden pre-activation at least m from 0 in the five evaluations whose
derivative enters a gradient (the actor at obs, q1 and q2 at obs | action, q1 and q2 at obs | a_pi under the stepped critics), m = 4 x
the largest deviation of torch-float32's hidden pre-activations from float64's on that case.  `settle` takes the rows inside a margin
out through `use`; a case may lose at most 20 % of its rows that way and must keep one (asserted in `reference`).

The deviation is taken with both precisions on the SAME parameters: in each of the five evaluations the float32 tower is the float64
tower of that moment rounded to float32, fed the float64 input rounded to float32.  Comparing the two torch runs' own stepped critics
instead measures something else: Adam's first step is lr sign(g), a critic entry whose gradient rounds to the other side of zero in
float32 lands 2 lr away, and the stepped critics' pre-activations then differ by 1e-4 and more - a margin that takes 52 of 63 rows at
(30, 4, 256, 3) and could not stay inside the cap.  With equal parameters the margin is 1e-6 to 5e-6, the figure the cap was set for;
what the stepped critics' own difference does to dq/da and to the actor's gradient is inside Y, as in DESIGN.md 23."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import policy_host as PH
import sac_host as SH

ROOT = PH.ROOT
DIR = os.path.join(ROOT, "tests", "hostbuild_sacw")
# (D, A, hidden, n_hidden, activation): the rows of the issue's table
SHAPE_A, SHAPE_REF = (14, 4, 128, 2, "relu"), (30, 4, 256, 3, "relu")
CASES = [(SHAPE_A, B) for B in (1, 63, 65, 200)] + [(SHAPE_REF, B) for B in (1, 63, 65, 200)] + \
    [((29, 1, 192, 3, "tanh"), 65), ((88, 8, 256, 2, "tanh"), 65), ((88, 8, 256, 3, "relu"), 65)]
CROSS = ((14, 4, 64, 2, "tanh"), 65)            # wide=True on the 64-64 tanh shape
ACTS = {"tanh": 0, "relu": 1}
MAX_SPLIT = 16
_lib = None
_refs = {}


def case_id(c):
    (D, A, H, L, act), B = c
    return "D%d-A%d-%dx%d-%s-B%d" % (D, A, H, L, act, B)


def sources():
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    return [os.path.join(DIR, "sacw_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + \
        [os.path.join(csrc, h) for h in ("xarm_sacw_core.h", "xarm_sac_core.h", "xarm_opt_core.h", "xarm_a2c_core.h", "xarm_policy_core.h",
                                         "xarm_norm_core.h", "xarm_core.h")]


def gxx_flags():
    """policy_host's flags with the loops over independent outputs vectorised (each output's chain keeps its order)"""
    return [f for f in PH.gxx_flags() if f != "-O1"] + ["-O3"]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "libsacw_host.so")
    srcs = sources()
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + gxx_flags() + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.swh_workspace_bytes.argtypes = L.swh_param_count.argtypes = [vp]
    L.swh_workspace_bytes.restype = L.swh_param_count.restype = C.c_int64
    L.swh_geometry.argtypes = L.swh_work_offsets.argtypes = [vp, vp]
    L.swh_act.argtypes = [vp] * 8
    L.swh_update.argtypes = [vp] * 20
    _lib = L
    return L


def abi_layout(B, shape, row_offset=0):
    from gym_xarm_amd import _native
    D, A, H, L, act = shape
    return _native.XarmSACWLayout(B, D, A, H, L, ACTS[act] if isinstance(act, str) else act, row_offset)


def abi_weights(ws, tp=None):
    """an xarm_sacw_weights over aligned arrays: module_params' 5 tp + 1 (or the trained 3 tp + 1; None entries stay NULL)"""
    from gym_xarm_amd import _native
    n = len(ws) - 1
    if tp is None:
        tp = n // 5 if n % 5 == 0 and n // 5 in (6, 8) else n // 3
    s = _native.XarmSACWWeights()
    for i, a in enumerate(ws):
        if a is None:
            continue
        if i == n:
            s.log_alpha = a.ctypes.data
        else:
            getattr(s, SH.TOWERS[i // tp])[i % tp] = a.ctypes.data
    return s


def geometry(B, shape):
    out = np.zeros(8 + MAX_SPLIT + 1 + 27, np.int64)
    lib().swh_geometry(C.byref(abi_layout(B, shape)), C.c_void_p(out.ctypes.data))
    nt = int(out[7])
    return {"S": int(out[0]), "max_split": int(out[1]), "split_rows": int(out[2]), "Pa": int(out[3]), "Pq": int(out[4]), "launches": int(out[5]),
            "act_launches": int(out[6]), "NT": nt, "rows": [int(v) for v in out[8:8 + MAX_SPLIT + 1]],
            "off": [int(v) for v in out[8 + MAX_SPLIT + 1:8 + MAX_SPLIT + 1 + nt + 1]]}


def model_tensors(model):
    from gym_xarm_amd.device_sac import module_params
    return module_params(model)


def trained_of(seq):
    from gym_xarm_amd.device_sac import trained
    return list(trained(tuple(seq)))


def sizes(model):
    return [int(t.numel()) for t in trained_of(model_tensors(model))]


def groups(model):
    tp = (len(model_tensors(model)) - 1) // 5
    return (("actor", slice(0, tp)), ("critic", slice(tp, 3 * tp)), ("log_alpha", slice(3 * tp, 3 * tp + 1)))


def split(flat, sz):
    o = np.cumsum([0] + list(sz))
    return [flat[o[i]:o[i + 1]] for i in range(len(sz))]


def weights_of(model):
    return [PH.aligned(t.detach().cpu().numpy()) for t in model_tensors(model)]


def zeros_like_trained(w):
    return [PH.aligned(np.zeros_like(a)) for a in trained_of(w)]


def fresh_state(model):
    w = weights_of(model)
    return w, zeros_like_trained(w), zeros_like_trained(w), np.zeros(1, np.int64)


def flat_of(ws):
    return np.concatenate([np.asarray(a, np.float64).ravel() for a in ws])


def model_flat(model, which="trained"):
    ts = model_tensors(model)
    tp = (len(ts) - 1) // 5
    ts = trained_of(ts) if which == "trained" else ts[3 * tp:5 * tp]
    return np.concatenate([t.detach().cpu().numpy().astype(np.float64).ravel() for t in ts])


def make_model(shape, seed=0):
    """SacPolicy(net_arch, activation)'s own initialisation under a fixed seed, the targets moved off the critics by a tenth of their
    spread, log_alpha -0.7"""
    from gym_xarm_amd.sac import SacPolicy
    D, A, H, L, act = shape
    g = torch.random.get_rng_state()
    torch.manual_seed(4177 + 31 * D + A + 7 * H + L + seed)
    model = SacPolicy(D, A, (H,) * L, act)
    ts = model_tensors(model)
    tp = (len(ts) - 1) // 5
    with torch.no_grad():
        for t, c in zip(ts[3 * tp:5 * tp], ts[tp:3 * tp]):
            t.copy_(c + 0.1 * c.abs().max() * torch.randn_like(c))
        model.log_alpha.fill_(-0.7)
    torch.random.set_rng_state(g)
    return model


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def workspace(B, shape):
    n = lib().swh_workspace_bytes(C.byref(abi_layout(B, shape)))
    assert n > 0
    return PH.aligned(np.zeros(n // 4 + 4, np.float32))


def host_update(w, m, v, step, b, h, shape, noise=True):
    """one step of the host build, in place on the aligned arrays of w, m, v and on step (int64 [1]); returns (rc, outputs)"""
    B, A = b["obs"].shape[0], shape[1]
    P = int(sum(a.size for a in trained_of(w)))
    out = {"grad": np.full(P, np.nan, np.float32), "dqda": np.full((2, B, A), np.nan, np.float32), "y": np.full(B, np.nan, np.float32),
           "stats": np.full(8, np.nan, np.float32), "q": np.full((2, B), np.nan, np.float32)}
    work = workspace(B, shape)
    ws, ms, vs = abi_weights(w), abi_weights(m), abi_weights(v)
    rc = lib().swh_update(C.byref(abi_layout(B, shape)), C.byref(SH.abi_params(h, A)), C.byref(ws), C.byref(ms), C.byref(vs), _p(step), _p(b["obs"]),
                          _p(b["next_obs"]), _p(b["action"]), _p(b["reward"]), _p(b["done"]), _p(b["use"]), _p(b["z_pi"] if noise else None),
                          _p(b["z_next"] if noise else None), _p(work), *[_p(out[k]) for k in ("grad", "dqda", "y", "stats", "q")])
    out["work"] = work
    return rc, out


def work_rows(work, B, shape):
    """the per-row parts of a workspace (the host build's or the device's, as a float32 array) after a step: logp_pi [B], logp' [B],
    z_pi [B, A], a_pi [B, A], a' [B, A], y [B]"""
    D, A = shape[:2]
    o = np.zeros(6, np.int64)
    lib().swh_work_offsets(C.byref(abi_layout(B, shape)), C.c_void_p(o.ctypes.data))
    part = lambda k, n: np.asarray(work[int(o[k]):int(o[k]) + n])
    return {"logp_pi": part(0, B), "logp_next": part(1, B), "z_pi": part(2, B * A).reshape(B, A), "a_pi": part(3, B * (D + A)).reshape(B, D + A)[:, D:],
            "a_next": part(4, B * (D + A)).reshape(B, D + A)[:, D:], "y": part(5, B)}


def work_floats(B, shape):
    return lib().swh_workspace_bytes(C.byref(abi_layout(B, shape))) // 4


def host_act(w, obs, shape, h, deterministic=False, calls=None, row_offset=0, logp=True):
    B, A = obs.shape[0], shape[1]
    calls = np.zeros(1, np.int64) if calls is None else calls
    out = {"action": np.full((B, A), np.nan, np.float32), "logp": np.full(B, np.nan, np.float32) if logp else None}
    work = workspace(B, shape)              # held here for the length of the call
    rc = lib().swh_act(C.byref(abi_layout(B, shape, row_offset)), C.byref(SH.abi_params(h, A, deterministic)), C.byref(abi_weights(w)), _p(calls),
                       _p(obs), _p(work), _p(out["action"]), _p(out["logp"]))
    del work
    assert rc == 0
    return out


# ---- torch: sac_host.torch_step with the hidden pre-activations of the five evaluations recorded
def torch_step(model, opts, b, h):
    """sac_host.torch_step's record plus "pre": the hidden pre-activations [rows, units] of the actor at obs, q1 / q2 at obs | action and
    q1 / q2 at obs | a_pi (the stepped critics), and "q": q1, q2 at obs | action"""
    calls, hooks, evals = {}, [], {}
    for name in ("actor", "q1", "q2"):
        seq = getattr(model, name)
        linears = [m for m in seq if isinstance(m, torch.nn.Linear)][:-1]
        hooks.append(linears[0].register_forward_hook(lambda mod, i, o, key=name, seq=seq: evals.setdefault(key, []).append((copy.deepcopy(seq), i[0].detach().clone()))))
        for li, lin in enumerate(linears):
            hooks.append(lin.register_forward_hook(lambda mod, i, o, key=(name, li): calls.setdefault(key, []).append(o.detach().numpy().astype(np.float64))))
        last = [m for m in seq if isinstance(m, torch.nn.Linear)][-1]
        hooks.append(last.register_forward_hook(lambda mod, i, o, key=(name, "out"): calls.setdefault(key, []).append(o.detach().numpy().astype(np.float64))))
    try:
        rec = SH.torch_step(model, opts, b, h)
    finally:
        for k in hooks:
            k.remove()
    # torch_step's order of calls: the actor on obs then on next_obs; each critic on obs | action, then (stepped) on obs | a_pi
    pre, start = [], []
    for (name, li), outs in calls.items():
        if li == "out":
            continue
        pre += [outs[0]] if name == "actor" else [outs[0], outs[1]]
        start += [np.ones(outs[0].shape[1], bool)] + ([] if name == "actor" else [np.zeros(outs[0].shape[1], bool)])
    rec["pre"] = np.concatenate(pre, axis=1)
    rec["pre_start"] = np.concatenate(start)          # the columns of the three evaluations at the call's own parameters
    if model.log_alpha.dtype == torch.float64:
        # the same evaluations in float32 on the same parameters and inputs, both rounded to float32
        pre32 = []
        for name in ("actor", "q1", "q2"):
            for seq, x in (evals[name][:1] if name == "actor" else evals[name][:2]):
                seq = seq.float()
                hs, xx = [], x.float()
                with torch.no_grad():
                    for mod in list(seq)[:-1]:
                        xx = mod(xx)
                        if isinstance(mod, torch.nn.Linear):
                            hs.append(xx.numpy().astype(np.float64))
                pre32.append(hs)
        # the order of `pre`: per tower, per layer, per evaluation
        order = []
        for ti, name in enumerate(("actor", "q1", "q2")):
            ev = pre32[0:1] if name == "actor" else (pre32[1:3] if name == "q1" else pre32[3:5])
            for li in range(len(ev[0])):
                order += [e[li] for e in ev]
        rec["pre32"] = np.concatenate(order, axis=1)
    rec["q"] = np.stack([calls[("q1", "out")][0][:, 0], calls[("q2", "out")][0][:, 0]])
    return rec


def torch_steps(model, batches, h, dtype):
    m = copy.deepcopy(model).to(dtype)
    opts = SH.make_opts(m, h)
    return m, opts, [torch_step(m, opts, b, h) for b in batches]


def margin(r32, r64):
    """the ReLU margin of a case: 4 x the largest deviation of float32's hidden pre-activations from float64's"""
    return 4.0 * np.abs(r64["pre32"] - r64["pre"]).max()


def near_rows(model, r32, r64, factor=1.0, evals="all"):
    """bool [B]: used rows inside a margin - sac_host.settle's two conditions and, for ReLU, a hidden pre-activation within `factor` x
    the margin of 0.  evals "start": only the three evaluations at the call's own parameters (the actor at obs, q1 and q2 at
    obs | action) - all that the critics' and log_alpha's gradients pass through"""
    q1, q2 = r64["qpi"]
    near = (np.abs(q1 - q2) < 1e-3 * factor * np.maximum(np.maximum(np.abs(q1), np.abs(q2)), 1.0)) | \
        (np.minimum(np.abs(r64["raw_log_std"] + 20.0), np.abs(r64["raw_log_std"] - 2.0)).min(1) < 1e-3 * factor)
    if model.activation == "relu":
        cols = r64["pre_start"] if evals == "start" else np.ones(r64["pre"].shape[1], bool)
        near |= np.abs(r64["pre"][:, cols]).min(1) < factor * margin(r32, r64)
    return near & (r64["use"] != 0)


def settle(model, b, h, evals="all"):
    """rows inside a margin (1.5 x the margin asserted afterwards, as sac_host.settle leaves room: masking a row moves the stepped critics a
    little) are taken out of the batch through `use`; returns the batch"""
    for _ in range(12):                 # thousands of rows: each pass moves the stepped critics by less, a few rows follow
        r64, r32 = torch_steps(model, [b], h, torch.float64)[2][0], torch_steps(model, [b], h, torch.float32)[2][0]
        near = near_rows(model, r32, r64, 1.0, evals)
        if not near.any():
            return b
        use = np.ones(near.shape, np.float32) if b["use"] is None else b["use"].copy()
        use[near] = 0.0
        b = dict(b, use=use)
    return b


def assert_valid(model, r32, r64, evals="all"):
    SH.assert_valid(r64)
    if model.activation == "relu":
        assert not near_rows(model, r32, r64, 1.0, evals).any(), "invalid case: a used row has a hidden pre-activation inside the ReLU margin"


def yardstick(x32, x64, sz):
    y = 0.0
    for a, r in zip(split(np.asarray(x32, np.float64), sz), split(x64, sz)):
        m = np.abs(r).max()
        if m > 0.0:
            y = max(y, np.abs(a - r).max() / m)
    return y


def bounds(x64, Y, sz, grp):
    parts, out = split(x64, sz), []
    for _, sl in grp:
        floor = 2.0 ** -23 * max(np.abs(r).max() for r in parts[sl])
        out += [4.0 * Y * np.abs(r).max() + floor for r in parts[sl]]
    return out


def rule(x, x64, Y, sz, grp, keep=None):
    """{group: (worst error / bound over the group's tensors, worst error relative to the tensor's largest entry in units of Y)}"""
    keep = np.ones(x64.shape, bool) if keep is None else keep
    xs, rs, ks, bd = split(np.asarray(x, np.float64), sz), split(x64, sz), split(keep, sz), bounds(x64, Y, sz, grp)
    res = {}
    for name, sl in grp:
        worst, in_y = 0.0, 0.0
        for a, r, k, b in zip(xs[sl], rs[sl], ks[sl], bd[sl]):
            if not k.any():
                continue
            err = np.abs(a - r)[k].max()
            worst = max(worst, err / b if b > 0 else (0.0 if err == 0 else np.inf))
            if np.abs(r).max() > 0 and Y > 0:
                in_y = max(in_y, err / np.abs(r).max() / Y)
        res[name] = (worst, in_y)
    return res


def reference(shape, B, ent_coef="auto", seed=0, evals="all", lr=None):
    """the model, the settled batch, the float64 and float32 torch records of one step, the yardstick and the rows the settle step took
    out; computed once and only read.  B = 1: the first draw seed whose row stays.  evals: near_rows'.  lr: in place of the default
    1e-3 (0: the critics at the actor step are the critics at call start, in torch and in the build alike - `DeviceSAC.grad`'s lr = 0)"""
    key = (shape, B, ent_coef, seed, evals, lr)
    if key in _refs:
        return _refs[key]
    D, A = shape[0], shape[1]
    h = SH.hyper(ent_coef=ent_coef) if lr is None else SH.hyper(ent_coef=ent_coef, lr=lr)
    model = make_model(shape, seed)
    for s in range(seed, seed + 32):
        b0 = SH.make_batch(D, A, B, 1.0, masked=B > 1, seed=s)
        b = settle(model, b0, h, evals)
        used0 = B if b0["use"] is None else int((b0["use"] != 0).sum())
        used = B if b["use"] is None else int((b["use"] != 0).sum())
        if used >= 1 or B > 1:
            break
    lost = used0 - used
    assert used >= 1, "the case keeps no row"
    assert lost <= 0.2 * B, "the settle step took %d of %d rows: more than 20 %%" % (lost, B)
    r64, r32 = torch_steps(model, [b], h, torch.float64)[2][0], torch_steps(model, [b], h, torch.float32)[2][0]
    assert_valid(model, r32, r64, evals)
    sz = sizes(model)
    _refs[key] = dict(h=h, b=b, model=model, r64=r64, r32=r32, Y=yardstick(r32["grad"], r64["grad"], sz), sz=sz, grp=groups(model), lost=lost,
                      margin=margin(r32, r64))
    return _refs[key]


def check_step(out, ref, what, start_only=False):
    """gradients under the rule, y / dq/da / q under sac_host's block rule, stats under its stats rule; returns the figures in units of Y.
    start_only (a reference settled with evals "start"): the critics' and log_alpha's gradients, y, q and the stats that do not pass
    through the stepped critics"""
    r64, r32 = ref["r64"], ref["r32"]
    Y = ref["Y"]
    if start_only:      # the yardstick over the tensors that are judged
        tp = ref["grp"][0][1].stop
        Y = yardstick(np.concatenate(split(r32["grad"], ref["sz"])[tp:]), np.concatenate(split(r64["grad"], ref["sz"])[tp:]), ref["sz"][tp:])
    res = rule(out["grad"], r64["grad"], Y, ref["sz"], ref["grp"])
    if start_only:
        res.pop("actor")
    fig = {k: v[1] for k, v in res.items()}
    for k, (worst, in_y) in res.items():
        assert worst <= 1.0, "%s: %s gradient %.2f x its bound (%.1f Y)" % (what, k, worst, in_y)
    used = r64["use"] != 0
    for k, x, a32, a64 in (("y", out["y"], r32["y"], r64["y"]), ("q", out["q"], r32["q"], r64["q"]),
                           ("dqda", out["dqda"][:, used], r32["dqda"][:, used], r64["dqda"][:, used])):
        if a64.size == 0 or (start_only and k == "dqda"):
            continue
        worst, in_y, _ = SH.block_rule(x, a32, a64)
        fig[k] = in_y
        assert worst <= 1.0, "%s: %s %.2f x its bound (%.1f Y)" % (what, k, worst, in_y)
    # sac_host's stats rule (tests/test_sac_host.py host_case): a row's terms pass through fewer than 16 + 8 A float32 roundings, the sums
    # run in float64.  A critic's output is a sum of terms whose sizes add up to at most (|W_out|_1 + |b_out|) max|h|; tanh keeps |h| <= 1,
    # ReLU does not, so the largest hidden pre-activation of the case (at least 1) scales it
    ref64, model, A = r64["stats"], ref["model"], ref["model"].act_dim
    rel = 4.0 * ref["Y"] + (16 + 8 * A) * 2.0 ** -24
    hmax = max(1.0, float(np.abs(r64["pre"]).max())) if model.activation == "relu" else 1.0
    last = lambda t: t[len(t) - 1]
    l1 = hmax * max(float((last(t).weight.abs().sum() + last(t).bias.abs().sum()).detach()) for t in (model.q1, model.q2, model.q1_target, model.q2_target))
    dq = rel * (2.0 * l1 + ref64["logp_abs"] + 1.0)
    tol = {"critic_loss": rel * ref64["critic_loss"] + 2.0 * np.sqrt(2.0 * ref64["critic_loss"]) * dq, "actor_loss": rel * ref64["actor_abs"] + dq,
           "alpha_loss": rel * abs(ref64["alpha_loss"]) + rel * ref64["logp_abs"], "alpha": 2.0 ** -22 * ref64["alpha"], "logp_pi": rel * ref64["logp_abs"],
           "min_q": rel * ref64["q_abs"] + dq, "n_use": 0.0}
    for i, k in enumerate(SH.STATS):
        if start_only and k in ("actor_loss", "min_q"):
            continue
        assert abs(float(out["stats"][i]) - ref64[k]) <= tol[k] + 2.0 ** -24 * abs(ref64[k]), (what, k, out["stats"][i], ref64[k], tol[k])
    assert out["stats"][7] == 0.0
    return fig


def check_rows(work, ref, B, shape, what):
    """a_pi, logp_pi, a' and logp' as the update's actor passes left them in the workspace, against float64 under sac_host's block rule
    (a', logp' have no float32 torch record: they are held to the float32 figure of a_pi / logp_pi)"""
    rows = work_rows(work, B, shape)
    r64, r32 = ref["r64"], ref["r32"]
    for k in ("a_pi", "logp_pi"):
        worst, in_y, _ = SH.block_rule(rows[k], r32[k], r64[k])
        assert worst <= 1.0, "%s: %s through the update %.2f x its bound" % (what, k, worst)
    assert np.array_equal(rows["z_pi"], ref["b"]["z_pi"]) and np.isfinite(rows["a_next"]).all() and np.abs(rows["a_next"]).max() <= 1.0
    return rows


def parameter_case(shape, B, n_steps, runner, cap, seed=0):
    """sac_host.parameter_case for any shape: float64 and float32 torch over n_steps whole steps (each step's draw settled under the
    float64 model as it stands), `runner(model, batches, h)` -> (flat trained parameters, flat targets), DESIGN.md 23's parameter rule on
    the entries kept - those whose float64 gradient lies outside the gradient rule's bound of zero at every step, or is exactly zero (a
    ReLU unit that is off on every used row by at least the margin: zero in float32 too, Adam leaves it alone).  cap: the share of a
    tensor that may be left out, asserted.  Returns (rule figures, Y, largest share left out, worst target error / bound)"""
    D, A = shape[:2]
    h = SH.hyper()
    model = make_model(shape, seed)
    sz, grp = sizes(model), groups(model)
    batches = [SH.make_batch(D, A, B, 1.0, True, seed=10 * seed + s) for s in range(n_steps)]
    for i in range(n_steps):
        mi = torch_steps(model, batches[:i], h, torch.float64)[0]
        batches[i] = settle(mi.float(), batches[i], h)
    m64, _, r64 = torch_steps(model, batches, h, torch.float64)
    m32, _, r32 = torch_steps(model, batches, h, torch.float32)
    left = np.zeros(sum(sz), bool)
    for s64, s32 in zip(r64, r32):
        Yg = yardstick(s32["grad"], s64["grad"], sz)
        left |= np.concatenate([(np.abs(r) <= bd) & (r != 0.0) for r, bd in zip(split(s64["grad"], sz), bounds(s64["grad"], Yg, sz, grp))])
    share = max(part.sum() / part.size for part in split(left, sz))
    assert share <= cap, "the reference leaves out %.2f %% of a tensor's entries: more than %.2f %%" % (100 * share, 100 * cap)
    p, tq = runner(model, batches, h)
    p64, p32 = model_flat(m64), model_flat(m32)
    keep = ~left
    Y = yardstick(np.where(keep, p32, p64), p64, sz)
    res = rule(p, p64, Y, sz, grp, keep)
    assert np.abs(p - model_flat(model)).max() > 1e-4                     # the steps moved the parameters
    # the targets: a target entry follows its critic entry with weight tau per step, under the same rule on the critic-shaped tensors
    t64, t32 = model_flat(m64, "targets"), model_flat(m32, "targets")
    tp = grp[0][1].stop
    qs = sz[tp:3 * tp]
    kq = np.concatenate(split(keep, sz)[tp:3 * tp])
    worst_t = 0.0
    for a, a32, a64, k in zip(split(np.asarray(tq, np.float64), qs), split(t32, qs), split(t64, qs), split(kq, qs)):
        m = np.abs(a64).max()
        Yt = np.abs(np.where(k, a32, a64) - a64).max() / m
        bound = 4.0 * Yt * m + 2.0 ** -23 * np.abs(t64).max()
        worst_t = max(worst_t, np.abs(a - a64)[k].max() / bound)
    return res, Y, share, worst_t
