"""ctypes view of tests/hostbuild_sac (g++ -ffp-contract=off build of csrc/xarm_sac_core.h) - CPU-side tests only - with the models,
the batches, a torch restatement (float64 / float32) of one SAC step of DESIGN.md 23 fed the same z, and the tolerance rule that the
host and GPU tests of the SAC update share.  Rows come from a2c_host.make_batch, the rule is a2c_host's over the 19
trained tensors: per tensor max|g - g64| <= 4 Y max|g64_tensor| + 2^-23 max|g64_group|, where the groups are the three optimisers'
(actor, both critics, log_alpha) and Y is what torch's own float32 autograd loses against float64 on the same case (the largest
relative loss over the 19 tensors: one figure per case, so that log_alpha's one-entry tensor is not judged by its own luck)."""
import copy
import ctypes as C
import math
import os
import subprocess

import numpy as np
import torch

import a2c_host as AH
import policy_host as PH

ROOT = PH.ROOT
DIR = os.path.join(ROOT, "tests", "hostbuild_sac")
WIDTHS = ((14, 4), (30, 4), (29, 1), (88, 8))          # Reach, PickAndPlace, an odd width with one action, D + A = 96 and 2 A = 16
ROWS = (1, 31, 33, 64, 65, 200)
HYPER = ("gamma", "lr", "tau", "ent_coef", "target_entropy", "beta1", "beta2", "eps")
DEFAULTS = dict(gamma=0.95, lr=1e-3, tau=0.005, ent_coef="auto", target_entropy=None, beta1=0.9, beta2=0.999, eps=1e-8, seed=0)
TOWERS = ("actor", "q1", "q2", "q1_target", "q2_target")
NAMES = tuple("%s_%s" % (t, k) for t in TOWERS for k in ("w1", "b1", "w2", "b2", "w3", "b3")) + ("log_alpha",)
TRAINED = NAMES[:18] + NAMES[30:]
GROUPS = (("actor", slice(0, 6)), ("critic", slice(6, 18)), ("log_alpha", slice(18, 19)))
STATS = ("critic_loss", "actor_loss", "alpha_loss", "alpha", "logp_pi", "min_q", "n_use")
_lib = None
_refs = {}


def sources():
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    return [os.path.join(DIR, "sac_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + \
        [os.path.join(csrc, h) for h in ("xarm_sac_core.h", "xarm_opt_core.h", "xarm_a2c_core.h", "xarm_policy_core.h", "xarm_norm_core.h", "xarm_core.h")]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "libsac_host.so")
    srcs = sources()
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + PH.gxx_flags() + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.sh_workspace_bytes.argtypes = L.sh_param_count.argtypes = [vp]
    L.sh_workspace_bytes.restype = L.sh_param_count.restype = C.c_int64
    L.sh_geometry.argtypes = [vp, vp]
    L.sh_act.argtypes = [vp] * 7
    L.sh_update.argtypes = [vp] * 19
    _lib = L
    return L


def hyper(**kw):
    h = dict(DEFAULTS)
    h.update(kw)
    return h


def abi_params(h, A, deterministic=False):
    from gym_xarm_amd import _native
    auto = h["ent_coef"] == "auto"
    vals = dict(h, ent_coef=0.0 if auto else float(h["ent_coef"]), target_entropy=-float(A) if h["target_entropy"] is None else h["target_entropy"])
    return _native.XarmSACParams(*([int(h["seed"])] + [float(vals[k]) for k in HYPER] + [int(auto), int(deterministic)]))


def abi_layout(B, D, A, row_offset=0):
    from gym_xarm_amd import _native
    return _native.XarmSACLayout(B, D, A, 64, row_offset)


def abi_weights(w, names=NAMES):
    """an xarm_sac_weights over the aligned arrays of w (missing names stay NULL)"""
    from gym_xarm_amd import _native
    s = _native.XarmSACWeights()
    for i, k in enumerate(NAMES):
        if k in names and w.get(k) is not None:
            if i == 30:
                s.log_alpha = w[k].ctypes.data
            else:
                getattr(s, TOWERS[i // 6])[i % 6] = w[k].ctypes.data
    return s


def geometry(B, D, A):
    """tiles, groups, rows per tile, the most groups, actor parameters, parameters of one critic, launches"""
    out = np.zeros(7, np.int64)
    lib().sh_geometry(C.byref(abi_layout(B, D, A)), C.c_void_p(out.ctypes.data))
    return [int(v) for v in out]


def sizes(D, A):
    """the 19 trained tensors"""
    q = [64 * (D + A), 64, 4096, 64, 64, 1]
    return [64 * D, 64, 4096, 64, 128 * A, 2 * A] + q + q + [1]


def split(flat, D, A):
    o = np.cumsum([0] + sizes(D, A))
    return [flat[o[i]:o[i + 1]] for i in range(19)]


def model_tensors(model):
    from gym_xarm_amd.device_sac import module_params
    return module_params(model)


def weights_of(model):
    """the model's 31 tensors as aligned NumPy arrays, by name"""
    return {k: PH.aligned(t.detach().cpu().numpy()) for k, t in zip(NAMES, model_tensors(model))}


def flat_of(w, names=TRAINED):
    return np.concatenate([np.asarray(w[k], np.float64).ravel() for k in names])


def model_flat(model, names=TRAINED):
    t = dict(zip(NAMES, model_tensors(model)))
    return np.concatenate([t[k].detach().numpy().astype(np.float64).ravel() for k in names])


def zeros_like_weights(w):
    return {k: PH.aligned(np.zeros_like(w[k])) for k in TRAINED}


def make_model(D, A, scale=1.0, seed=0):
    """SacPolicy's own initialisation under a fixed seed, every weight and bias of the towers multiplied by `scale` (4: the tanh
    saturates), the targets moved off the critics by a tenth of their spread, log_alpha -0.7"""
    from gym_xarm_amd.sac import SacPolicy
    g = torch.random.get_rng_state()
    torch.manual_seed(977 + 31 * D + A + seed)
    model = SacPolicy(D, A)
    with torch.no_grad():
        for t in model_tensors(model)[:18]:
            t.mul_(scale)
        for t, c in zip(model_tensors(model)[18:30], model_tensors(model)[6:18]):
            t.copy_(c + 0.1 * c.abs().max() * torch.randn_like(c))
        model.log_alpha.fill_(-0.7)
    torch.random.set_rng_state(g)
    return model


def make_batch(D, A, B, scale, masked=True, seed=0):
    """a2c_host.make_batch's draws for two steps of B envs: step 0's rows are obs, step 1's next_obs; its standard normal actions of step
    0, squashed, are the stored actions (a replay buffer holds tanh outputs) and those of step 1 are z_pi; z_next is a draw of its own"""
    b = AH.make_batch(D, A, 2, B, scale, masked, seed)
    rs = np.random.RandomState(555 + 7 * D + A + 13 * B + seed)
    c = np.ascontiguousarray
    return {"obs": c(b["obs"][0]), "next_obs": c(b["obs"][1]), "action": c(np.tanh(b["action"][0]).astype(np.float32)), "reward": c(b["reward"][0]),
            "done": c(b["done"][0]), "use": None if b["use"] is None else c(b["use"][0]), "z_pi": c(b["action"][1]),
            "z_next": rs.standard_normal((B, A)).astype(np.float32)}


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def host_update(w, m, v, step, b, h, noise=True):
    """one step of the host build, in place on the aligned arrays of w (31), m and v (19) and on step (int64 [1]); returns (rc, outputs)"""
    B, D = b["obs"].shape
    A = b["action"].shape[1]
    P = sum(sizes(D, A))
    out = {"grad": np.full(P, np.nan, np.float32), "dqda": np.full((2, B, A), np.nan, np.float32), "y": np.full(B, np.nan, np.float32),
           "stats": np.full(8, np.nan, np.float32)}
    work = PH.aligned(np.zeros(4, np.float32))
    ws, ms, vs = abi_weights(w), abi_weights(m, TRAINED), abi_weights(v, TRAINED)
    rc = lib().sh_update(C.byref(abi_layout(B, D, A)), C.byref(abi_params(h, A)), C.byref(ws), C.byref(ms), C.byref(vs), _p(step), _p(b["obs"]),
                         _p(b["next_obs"]), _p(b["action"]), _p(b["reward"]), _p(b["done"]), _p(b["use"]), _p(b["z_pi"] if noise else None),
                         _p(b["z_next"] if noise else None), _p(work), *[_p(out[k]) for k in ("grad", "dqda", "y", "stats")])
    return rc, out


def host_act(w, obs, A, h, deterministic=False, calls=None, row_offset=0, logp=True):
    B, D = obs.shape
    calls = np.zeros(1, np.int64) if calls is None else calls
    out = {"action": np.full((B, A), np.nan, np.float32), "logp": np.full(B, np.nan, np.float32) if logp else None}
    rc = lib().sh_act(C.byref(abi_layout(B, D, A, row_offset)), C.byref(abi_params(h, A, deterministic)), C.byref(abi_weights(w)), _p(calls), _p(obs),
                      _p(out["action"]), _p(out["logp"]))
    assert rc == 0
    return out


def fresh_state(model):
    """(w, m, v, step) for the host build: the model's weights, zero Adam state"""
    w = weights_of(model)
    return w, zeros_like_weights(w), zeros_like_weights(w), np.zeros(1, np.int64)


# ---- torch: one SAC step of DESIGN.md 23 in the model's dtype, restated loss by loss
def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def actor_row(model, obs, z, deterministic=False):
    """(a, logp, raw log_std) of the squashed Gaussian"""
    A = model.act_dim
    out = model.actor(obs)
    mean, raw = out[:, :A], out[:, A:]
    ls = raw.clamp(-20.0, 2.0)
    a = torch.tanh(mean if deterministic else mean + ls.exp() * z)
    zz = torch.zeros_like(mean) if deterministic else z
    logp = (-0.5 * zz * zz - ls - 0.5 * math.log(2.0 * math.pi)).sum(-1) - torch.log(1.0 - a * a + 1e-6).sum(-1)
    return a, logp, raw


def make_opts(model, h):
    kw = dict(lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
    return {"actor": torch.optim.Adam(model.actor.parameters(), **kw), "critic": torch.optim.Adam(model.critic_parameters(), **kw),
            "alpha": torch.optim.Adam([model.log_alpha], **kw) if h["ent_coef"] == "auto" else None}


def torch_step(model, opts, b, h):
    """one SAC step in place on `model` (any dtype) with the three Adams `opts`; returns the record of the step: the flat float64
    gradient of the 19 trained tensors, y, dq/da, a_pi, logp_pi, q(obs | a_pi), the actor's raw log_std and the stats"""
    dt = model.log_alpha.dtype
    A = model.act_dim
    obs, nobs, act, rew, done, z_pi, z_next = (_t(b[k], dt) for k in ("obs", "next_obs", "action", "reward", "done", "z_pi", "z_next"))
    use = torch.ones_like(rew) if b["use"] is None else _t(b["use"], dt)
    n_use = use.sum().clamp(min=1.0)
    mean = lambda x: (x * use).sum() / n_use
    auto = h["ent_coef"] == "auto"
    te = -float(A) if h["target_entropy"] is None else float(h["target_entropy"])
    alpha = model.log_alpha.detach().exp().squeeze() if auto else torch.tensor(float(h["ent_coef"]), dtype=dt)
    a_pi, logp_pi, raw = actor_row(model, obs, z_pi)
    alpha_loss = -mean(model.log_alpha.squeeze() * (logp_pi.detach() + te)) if auto else torch.zeros((), dtype=dt)
    g_alpha = torch.autograd.grad(alpha_loss, model.log_alpha)[0] if auto else torch.zeros(1, dtype=dt)
    with torch.no_grad():
        a_next, logp_next, _ = actor_row(model, nobs, z_next)
        q1t, q2t = model.q_values(nobs, a_next, target=True)
        y = rew + h["gamma"] * (1.0 - done) * (torch.minimum(q1t, q2t) - alpha * logp_next)
    q1, q2 = model.q_values(obs, act)
    critic_loss = 0.5 * (mean((q1 - y) ** 2) + mean((q2 - y) ** 2))
    cp = model.critic_parameters()
    g_critic = torch.autograd.grad(critic_loss, cp)
    for p, g in zip(cp, g_critic):
        p.grad = g
    opts["critic"].step()
    q1p, q2p = model.q_values(obs, a_pi)
    dq1, dq2 = torch.autograd.grad(q1p.sum(), a_pi, retain_graph=True)[0], torch.autograd.grad(q2p.sum(), a_pi, retain_graph=True)[0]
    qmin = torch.minimum(q1p, q2p)
    actor_loss = mean(alpha * logp_pi - qmin)
    ap = list(model.actor.parameters())
    g_actor = torch.autograd.grad(actor_loss, ap)
    for p, g in zip(ap, g_actor):
        p.grad = g
    opts["actor"].step()
    if auto:
        model.log_alpha.grad = g_alpha
        opts["alpha"].step()
    with torch.no_grad():
        for t, c in zip(list(model.q1_target.parameters()) + list(model.q2_target.parameters()), cp):
            t.copy_(torch.lerp(t, c, h["tau"]))
    n = lambda x: x.detach().numpy().astype(np.float64)
    f = lambda x: float(x.detach())
    grad = np.concatenate([n(g).ravel() for g in list(g_actor) + list(g_critic) + [g_alpha]])
    return {"grad": grad, "y": n(y), "dqda": np.stack([n(dq1), n(dq2)]), "a_pi": n(a_pi), "logp_pi": n(logp_pi), "qpi": np.stack([n(q1p), n(q2p)]),
            "raw_log_std": n(raw), "use": n(use),
            "stats": {"critic_loss": f(critic_loss), "actor_loss": f(actor_loss), "alpha_loss": f(alpha_loss), "alpha": f(alpha), "logp_pi": f(mean(logp_pi)),
                      "min_q": f(mean(qmin)), "n_use": f(n_use), "actor_abs": f(mean((alpha * logp_pi).abs() + qmin.abs())),
                      "logp_abs": f(mean(logp_pi.abs())), "q_abs": f(mean(qmin.abs()))}}


def torch_steps(model, batches, h, dtype):
    """the steps on a `dtype` copy; returns (model, opts, one record per step)"""
    m = copy.deepcopy(model).to(dtype)
    opts = make_opts(m, h)
    return m, opts, [torch_step(m, opts, b, h) for b in batches]


def assert_valid(rec):
    """the condition on a case's inputs, in float64: no used row has |q1 - q2| < 1e-4 max(|q1|, |q2|, 1) at the actor step (float32 and
    float64 then pick the same critic), none has a log_std output within 1e-4 of -20 or 2"""
    used = rec["use"] != 0
    if not used.any():
        return
    q1, q2 = rec["qpi"][0][used], rec["qpi"][1][used]
    gap = (np.abs(q1 - q2) / np.maximum(np.maximum(np.abs(q1), np.abs(q2)), 1.0)).min()
    raw = rec["raw_log_std"][used]
    edge = np.minimum(np.abs(raw + 20.0), np.abs(raw - 2.0)).min()
    assert gap >= 1e-4 and edge >= 1e-4, "invalid case: critics %.2e apart / a log_std %.2e from the clamp" % (gap, edge)


def reference(D, A, B, scale=1.0, ent_coef="auto", masked=True, shift=False):
    """the model, the batch, the float64 and float32 torch records of one step and the yardstick; computed once and only read.
    shift: the clamp case (clamp_model)"""
    key = (D, A, B, scale, ent_coef, masked, shift)
    if key not in _refs:
        h = hyper(ent_coef=ent_coef)
        b = make_batch(D, A, B, scale, masked)
        model = make_model(D, A, scale)
        if shift:
            model, b = clamp_model(model, b)
        b = settle(model, b, h)
        _, _, r64 = torch_steps(model, [b], h, torch.float64)
        _, _, r32 = torch_steps(model, [b], h, torch.float32)
        assert_valid(r64[0])
        _refs[key] = dict(h=h, b=b, model=model, r64=r64[0], r32=r32[0], Y=yardstick(r32[0]["grad"], r64[0]["grad"], D, A))
    return _refs[key]


def settle(model, b, h):
    """the draws are chosen so that the float64 reference alone meets assert_valid: a row whose critics lie within 1e-3 of each other at
    the actor step, or whose log_std lies within 1e-3 of a clamp edge, in float64, is taken out of the batch through `use` (about one
    row in a thousand; masking a row moves the stepped critics by less than the margin left)"""
    for _ in range(3):
        _, _, r = torch_steps(model, [b], h, torch.float64)
        r = r[0]
        q1, q2 = r["qpi"]
        near = (np.abs(q1 - q2) < 1e-3 * np.maximum(np.maximum(np.abs(q1), np.abs(q2)), 1.0)) | \
            (np.minimum(np.abs(r["raw_log_std"] + 20.0), np.abs(r["raw_log_std"] - 2.0)).min(1) < 1e-3)
        near &= r["use"] != 0
        if not near.any():
            return b
        use = np.ones(q1.shape, np.float32) if b["use"] is None else b["use"].copy()
        use[near] = 0.0
        b = dict(b, use=use)
    return b


def clamp_model(model, b):
    """the clamp case: the bias of the actor's log_std outputs shifted so that the rows n % 3 == 0 - a known third - sit beyond the upper
    clamp by at least 0.1 in every column (in float64); returns (model, batch with `use` = that third)"""
    m = copy.deepcopy(model)
    A = m.act_dim
    with torch.no_grad():
        raw = copy.deepcopy(m).double().actor(_t(b["obs"], torch.float64))[:, A:].numpy()
        third = np.arange(raw.shape[0]) % 3 == 0
        m.actor[4].bias[A:] += torch.from_numpy((2.1 - raw[third].min(0)).astype(np.float32)) + 1e-3
    return m, dict(b, use=third.astype(np.float32))


# ---- the rule
def yardstick(x32, x64, D, A):
    y = 0.0
    for a, r in zip(split(np.asarray(x32, np.float64), D, A), split(x64, D, A)):
        m = np.abs(r).max()
        if m > 0.0:
            y = max(y, np.abs(a - r).max() / m)
    return y


def bounds(x64, Y, D, A):
    """the rule's bound of each of the 19 tensors; the floor is 2^-23 of the largest entry of the tensor's optimiser group"""
    parts, out = split(x64, D, A), []
    for _, sl in GROUPS:
        floor = 2.0 ** -23 * max(np.abs(r).max() for r in parts[sl])
        out += [4.0 * Y * np.abs(r).max() + floor for r in parts[sl]]
    return out


def rule(x, x64, Y, D, A, keep=None):
    """{group: (worst error / bound over the group's tensors, worst error relative to the tensor's largest entry in units of Y)}"""
    keep = np.ones(x64.shape, bool) if keep is None else keep
    xs, rs, ks, bd = split(np.asarray(x, np.float64), D, A), split(x64, D, A), split(keep, D, A), bounds(x64, Y, D, A)
    res = {}
    for name, sl in GROUPS:
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


def block_rule(x, x32, x64):
    """a per-row quantity (y, dq/da) with the row block treated as one tensor: (error / bound, error in units of Y, Y)"""
    m = np.abs(x64).max()
    Y = np.abs(np.asarray(x32, np.float64) - x64).max() / m if m > 0 else 0.0
    err = np.abs(np.asarray(x, np.float64) - x64).max()
    bound = 4.0 * Y * m + 2.0 ** -23 * m
    return (err / bound if bound > 0 else (0.0 if err == 0 else np.inf)), (err / m / Y if m > 0 and Y > 0 else 0.0), Y


def sensitive(g64, Y, D, A):
    """bool [P]: gradient entries within the gradient rule's bound of zero - Adam's first steps are nearly lr sign(g), so their parameters
    are left out of the parameter comparison (at most 1 % of a tensor's entries may be)"""
    return np.concatenate([np.abs(r) <= bd for r, bd in zip(split(g64, D, A), bounds(g64, Y, D, A))])


def parameter_case(D, A, B, n_steps, runner, ent_coef="auto"):
    """whole steps: float64 and float32 torch, `runner(model, batches, h)` (the build under test: returns the flat trained parameters and
    the flat targets), and the entries left out - those whose float64 gradient lies within the gradient bound of zero at any step"""
    h = hyper(ent_coef=ent_coef)
    model = make_model(D, A, 1.0)
    batches = [make_batch(D, A, B, 1.0, True, seed=s) for s in range(n_steps)]
    for i in range(n_steps):            # each step's draw settled under the float64 model as it stands at that step
        mi = torch_steps(model, batches[:i], h, torch.float64)[0]
        batches[i] = settle(mi, batches[i], h)
    m64, _, r64 = torch_steps(model, batches, h, torch.float64)
    m32, _, r32 = torch_steps(model, batches, h, torch.float32)
    left_out = np.zeros(sum(sizes(D, A)), bool)
    for s64, s32 in zip(r64, r32):
        assert_valid(s64)
        left_out |= sensitive(s64["grad"], yardstick(s32["grad"], s64["grad"], D, A), D, A)
    for part in split(left_out, D, A):
        assert part.sum() <= 0.01 * part.size, "more than 1 % of a tensor's entries have a float64 gradient at zero"
    p, tq = runner(model, batches, h)
    p64, p32 = model_flat(m64), model_flat(m32)
    keep = ~left_out
    Y = yardstick(np.where(keep, p32, p64), p64, D, A)
    res = rule(p, p64, Y, D, A, keep)
    assert np.abs(p - model_flat(model)).max() > 1e-4                     # the steps moved the parameters
    # the targets: a target entry follows its critic entry with weight tau per step, under the same rule on the 12 critic-shaped tensors
    t64, t32 = model_flat(m64, NAMES[18:30]), model_flat(m32, NAMES[18:30])
    o = np.cumsum([0] + sizes(D, A))
    kq = keep[o[6]:o[18]]
    worst_t = 0.0
    q = sizes(D, A)[6:18]
    oq = np.cumsum([0] + q)
    for i in range(12):
        sl = slice(oq[i], oq[i + 1])
        k = kq[sl]
        m = np.abs(t64[sl]).max()
        Yt = np.abs(np.where(k, t32[sl], t64[sl]) - t64[sl]).max() / m
        bound = 4.0 * Yt * m + 2.0 ** -23 * np.abs(t64).max()
        worst_t = max(worst_t, np.abs(tq[sl] - t64[sl])[k].max() / bound)
    return res, Y, int(left_out.sum()), worst_t
