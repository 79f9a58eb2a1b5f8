"""ctypes view of tests/hostbuild_td3 (g++ -ffp-contract=off build of csrc/xarm_td3_core.h) - CPU-side tests only - with the models, the
cases, a torch restatement (float64 / float32) of one TD3 step of DESIGN.md 28 fed the same z, and sacw_host's tolerance rule over TD3's
trained tensors: per tensor max|g - g64| <= 4 Y max|g64_tensor| + 2^-23 max|g64_group|, the groups the two optimisers' (actor, both
critics), Y the largest relative loss of torch's float32 autograd against float64 over the case's trained tensors and its three row
blocks y, q and dq1/da (relative to the block's largest entry) - one figure per case, never a figure of the code under test.  The row
blocks are held to the same rule with the same Y, each block a group of its own.  One figure for all: at B = 1 a block is one or two
numbers, each the cancelling sum of a tower's output, which torch's float32 hits to the last bit or misses by 1e-5 of itself.

Validity: TD3's step has no branch on a tie that a gradient passes through (the target's min and clamps carry no gradient and are
continuous), so tanh cases need no condition.  For ReLU the derivative jumps at 0: a used row must have, in float64, every hidden
pre-activation at least m from 0 in the evaluations whose derivative enters a gradient - q1 and q2 at obs | action and, on a step with
an actor update, the actor at obs and the stepped q1 at obs | a_pi - with m = 4 x the largest deviation of float32's hidden
pre-activations from float64's, both precisions on the SAME parameters and inputs (sacw_host's reasoning).  `settle` takes the rows inside a
margin out through `use`; a case may lose at most 20 % of its rows that way and must keep one (asserted in `reference`).

The one-step cases start from a WARM optimiser state (`warm_state`: random exp_avg / exp_avg_sq and a step count of 4 policy_delay, what
training holds after its first steps).  From zero state Adam's step is lr g / (|g| + eps): an entry whose gradient is of the size of eps =
1e-8 lands anywhere in +- lr depending on the last bit of g, so the stepped q1 - and through it dq1/da and the actor's gradient - differs
between any two float32 orders of summation, torch's own included: over seeds 0 .. 3 the torch pair's Y for (30, 4, 256, 3) at 63 rows
ran from 3e-7 to 2e-5 and the stepped q1 of the two precisions lay up to 5e-5 apart.  From a warm state the step is continuous in g, the
stepped q1 agrees to 7e-9 and Y stays at 3e-7 .. 1.4e-6: the case measures the arithmetic, not the luck of a sign.  The cold start is
covered by the whole-step tests (parameter rule, which leaves such entries out) and by the bitwise comparison of device and host build."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import torch

import policy_host as PH
import sac_host as SH
import sacw_host as WH

ROOT = PH.ROOT
DIR = os.path.join(ROOT, "tests", "hostbuild_td3")
SHAPE_A, SHAPE_REF = WH.SHAPE_A, WH.SHAPE_REF
SHAPE_64 = (14, 4, 64, 2, "tanh")
CASES = [(SHAPE_A, B) for B in (1, 63, 65, 200)] + [(SHAPE_REF, B) for B in (1, 63, 65, 200)] + \
    [((29, 1, 192, 3, "tanh"), 65), ((88, 8, 256, 2, "tanh"), 65), (SHAPE_64, 65)]
HYPER = ("gamma", "lr", "tau", "beta1", "beta2", "eps", "target_policy_noise", "target_noise_clip", "action_noise")
DEFAULTS = dict(gamma=0.95, lr=1e-3, tau=0.005, beta1=0.9, beta2=0.999, eps=1e-8, target_policy_noise=0.2, target_noise_clip=0.5,
                action_noise=0.1, policy_delay=2, seed=0)
TOWERS = ("actor", "q1", "q2", "actor_target", "q1_target", "q2_target")
MODES = {"deterministic": 0, "gaussian": 1, "uniform": 2}
STATS = ("critic_loss", "actor_loss", "q1_pi", "target_q", "n_use", "actor_stepped")
MAX_SPLIT = 16
case_id = WH.case_id
_lib = None
_refs = {}


def sources():
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    return [os.path.join(DIR, "td3_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + \
        [os.path.join(csrc, h) for h in ("xarm_td3_core.h", "xarm_sacw_core.h", "xarm_sac_core.h", "xarm_opt_core.h", "xarm_a2c_core.h",
                                         "xarm_policy_core.h", "xarm_norm_core.h", "xarm_core.h")]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "libtd3_host.so")
    srcs = sources()
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++"] + WH.gxx_flags() + ["-fPIC", "-shared", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.t3h_workspace_bytes.argtypes = L.t3h_param_count.argtypes = [vp]
    L.t3h_workspace_bytes.restype = L.t3h_param_count.restype = C.c_int64
    L.t3h_geometry.argtypes = L.t3h_work_offsets.argtypes = [vp, vp]
    L.t3h_act.argtypes = [vp] * 7
    L.t3h_update.argtypes = [vp] * 19
    _lib = L
    return L


def hyper(**kw):
    h = dict(DEFAULTS)
    h.update(kw)
    return h


def abi_params(h, mode="deterministic"):
    from gym_xarm_amd import _native
    return _native.XarmTD3Params(*([int(h["seed"])] + [float(h[k]) for k in HYPER] + [int(h["policy_delay"]), MODES[mode]]))


abi_layout = WH.abi_layout


def abi_weights(ws):
    """an xarm_td3_weights over aligned arrays: module_params' 6 tp or the trained 3 tp (None entries stay NULL)"""
    from gym_xarm_amd import _native
    tp = len(ws) // (6 if len(ws) in (36, 48) else 3)
    s = _native.XarmTD3Weights()
    for i, a in enumerate(ws):
        if a is not None:
            getattr(s, TOWERS[i // tp])[i % tp] = a.ctypes.data
    return s


def geometry(B, shape):
    out = np.zeros(6 + MAX_SPLIT + 1, np.int64)
    lib().t3h_geometry(C.byref(abi_layout(B, shape)), C.c_void_p(out.ctypes.data))
    return {"S": int(out[0]), "Pa": int(out[1]), "Pq": int(out[2]), "launches": int(out[3]), "act_launches": int(out[4]), "NT": int(out[5]),
            "rows": [int(v) for v in out[6:]]}


def model_tensors(model):
    from gym_xarm_amd.device_td3 import module_params
    return module_params(model)


def trained_of(seq):
    return list(seq[:len(seq) // 2])


def sizes(model):
    return [int(t.numel()) for t in trained_of(model_tensors(model))]


def groups(model):
    tp = len(model_tensors(model)) // 6
    return (("actor", slice(0, tp)), ("critic", slice(tp, 3 * tp)))


def weights_of(model):
    return [PH.aligned(t.detach().cpu().numpy()) for t in model_tensors(model)]


def zeros_like_trained(w):
    return [PH.aligned(np.zeros_like(a)) for a in trained_of(w)]


def fresh_state(model, step=0):
    w = weights_of(model)
    return w, zeros_like_trained(w), zeros_like_trained(w), np.full(1, step, np.int64)


def ref_state(ref):
    """(w, m, v, step) for the host build at a reference's start: the model's weights and its warm optimiser state, copied"""
    return weights_of(ref["model"]), [PH.aligned(a.copy()) for a in ref["m"]], [PH.aligned(a.copy()) for a in ref["v"]], np.full(1, ref["step"], np.int64)


def flat_of(ws):
    return np.concatenate([np.asarray(a, np.float64).ravel() for a in ws])


def model_flat(model, which="trained"):
    ts = model_tensors(model)
    ts = ts[:len(ts) // 2] if which == "trained" else ts[len(ts) // 2:]
    return np.concatenate([t.detach().cpu().numpy().astype(np.float64).ravel() for t in ts])


def make_model(shape, seed=0):
    """Td3Policy(net_arch, activation)'s own initialisation under a fixed seed, every target moved off its net by a tenth of its spread"""
    from gym_xarm_amd.td3 import Td3Policy
    D, A, H, L, act = shape
    g = torch.random.get_rng_state()
    torch.manual_seed(5077 + 31 * D + A + 7 * H + L + seed)
    model = Td3Policy(D, A, (H,) * L, act)
    ts = model_tensors(model)
    with torch.no_grad():
        for t, c in zip(ts[len(ts) // 2:], ts[:len(ts) // 2]):
            t.copy_(c + 0.1 * c.abs().max() * torch.randn_like(c))
    torch.random.set_rng_state(g)
    return model


def make_batch(D, A, B, masked=True, seed=0):
    """sac_host.make_batch's rows (obs, next_obs, a stored action in [-1, 1], done, use, z_next) with the rewards of the sparse task the
    learner is for: -1 on four rows in five, else 0.  With rewards symmetric about 0 and a fresh critic the gradient of a critic's
    output bias - the mean of 2 (q - y) - cancels to a thousandth of its terms, and that one-entry tensor then measures the last bits of a
    sum in torch's float32 and in the build alike (its relative error sets Y or misses 4 Y by luck); with the task's rewards q - y has a
    decided sign"""
    b = SH.make_batch(D, A, B, 1.0, masked, seed)
    b.pop("z_pi")
    rs = np.random.RandomState(811 + 7 * D + A + 13 * B + seed)
    b["reward"] = np.ascontiguousarray(-(rs.uniform(size=B) < 0.8).astype(np.float32))
    return b


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def workspace(B, shape):
    n = lib().t3h_workspace_bytes(C.byref(abi_layout(B, shape)))
    assert n > 0
    return PH.aligned(np.zeros(n // 4 + 4, np.float32))


def work_floats(B, shape):
    return lib().t3h_workspace_bytes(C.byref(abi_layout(B, shape))) // 4


def host_update(w, m, v, step, b, h, shape, noise=True, stats=None, row_offset=0):
    """one step of the host build, in place on the aligned arrays of w, m, v and on step (int64 [1]); returns (launches or -1, outputs).
    stats: the row the call writes into (zeros when None) - actor_loss and q1_pi stay as they are on a call without an actor step"""
    B, A = b["obs"].shape[0], shape[1]
    P = int(sum(a.size for a in trained_of(w)))
    out = {"grad": np.zeros(P, np.float32), "y": np.full(B, np.nan, np.float32), "q": np.full((2, B), np.nan, np.float32),
           "dqda": np.zeros((B, A), np.float32), "stats": np.zeros(8, np.float32) if stats is None else stats}
    work = workspace(B, shape)
    ws, ms, vs = abi_weights(w), abi_weights(m), abi_weights(v)
    rc = lib().t3h_update(C.byref(abi_layout(B, shape, row_offset)), C.byref(abi_params(h)), C.byref(ws), C.byref(ms), C.byref(vs), _p(step), _p(b["obs"]),
                          _p(b["next_obs"]), _p(b["action"]), _p(b["reward"]), _p(b["done"]), _p(b["use"]), _p(b["z_next"] if noise else None),
                          _p(work), *[_p(out[k]) for k in ("grad", "y", "q", "dqda", "stats")])
    out["work"] = work
    return rc, out


def work_parts(work, B, shape):
    """parts of a workspace (the host build's or the device's, as a float32 array) after a step: the delay flag, a' [B, A], a_pi [B, A], y [B]"""
    D, A = shape[:2]
    o = np.zeros(4, np.int64)
    lib().t3h_work_offsets(C.byref(abi_layout(B, shape)), C.c_void_p(o.ctypes.data))
    part = lambda k, n: np.asarray(work[int(o[k]):int(o[k]) + n])
    return {"flag": int(part(0, 1).view(np.int32)[0]), "a_next": part(1, B * (D + A)).reshape(B, D + A)[:, D:],
            "a_pi": part(2, B * (D + A)).reshape(B, D + A)[:, D:], "y": part(3, B)}


def host_act(w, obs, shape, h, mode="deterministic", calls=None, row_offset=0):
    B, A = obs.shape[0], shape[1]
    calls = np.zeros(1, np.int64) if calls is None else calls
    out = np.full((B, A), np.nan, np.float32)
    work = workspace(B, shape)
    rc = lib().t3h_act(C.byref(abi_layout(B, shape, row_offset)), C.byref(abi_params(h, mode)), C.byref(abi_weights(w)), _p(calls), _p(obs), _p(work), _p(out))
    del work
    assert rc == 0
    return out


# ---- torch: one TD3 step of DESIGN.md 28 in the model's dtype, restated loss by loss, with the hidden pre-activations recorded
def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def tower_pre(seq, x):
    """(output, [hidden pre-activation per hidden layer]) of a tower"""
    pre = []
    mods = list(seq)
    for mod in mods[:-1]:
        x = mod(x)
        if isinstance(mod, torch.nn.Linear):
            pre.append(x)
    return mods[-1](x), pre


def make_opts(model, h):
    from gym_xarm_amd.td3 import make_optimizers
    return make_optimizers(model, h["lr"], (h["beta1"], h["beta2"]), h["eps"])


def torch_step(model, opts, b, h, n_updates):
    """one TD3 step in place on `model` (any dtype) with the two Adams `opts`; n_updates counts from 1 and includes this step.  Returns the
    record: the flat float64 gradient of the trained tensors (the actor's zero on a step without an actor update), y, q, dq1/da, a_pi,
    the hidden pre-activations of the evaluations whose derivative enters a gradient (and, for a float64 model, the same evaluations in
    float32 on the same parameters and inputs), use and the stats"""
    dt = model.actor[0].weight.dtype
    obs, nobs, act, rew, done, z = (_t(b[k], dt) for k in ("obs", "next_obs", "action", "reward", "done", "z_next"))
    use = torch.ones_like(rew) if b["use"] is None else _t(b["use"], dt)
    n_use = use.sum().clamp(min=1.0)
    mean = lambda x: (x * use).sum() / n_use
    evals = []                                                   # (tower as it is at that moment, its input)
    with torch.no_grad():
        noise = (h["target_policy_noise"] * z).clamp(-h["target_noise_clip"], h["target_noise_clip"])
        a_next = (model.action(nobs, target=True) + noise).clamp(-1.0, 1.0)
        q1t, q2t = model.q_values(nobs, a_next, target=True)
        y = rew + (1.0 - done) * h["gamma"] * torch.minimum(q1t, q2t)
    xq = torch.cat([obs, act], dim=-1)
    pre = []
    evals += [(copy.deepcopy(model.q1), xq), (copy.deepcopy(model.q2), xq)]
    q1, p1 = tower_pre(model.q1, xq)
    q2, p2 = tower_pre(model.q2, xq)
    q1, q2 = q1.squeeze(-1), q2.squeeze(-1)
    pre += p1 + p2
    critic_loss = mean((q1 - y) ** 2) + mean((q2 - y) ** 2)
    cp = model.critic_parameters()
    g_critic = torch.autograd.grad(critic_loss, cp)
    for p, g in zip(cp, g_critic):
        p.grad = g
    opts["critic"].step()
    ap = list(model.actor.parameters())
    stepped = n_updates % h["policy_delay"] == 0
    B, A = act.shape
    if stepped:
        evals.append((copy.deepcopy(model.actor), obs))
        out, pa = tower_pre(model.actor, obs)
        a_pi = torch.tanh(out)
        xpi = torch.cat([obs, a_pi], dim=-1)
        evals.append((copy.deepcopy(model.q1), xpi.detach()))
        q1p, pq = tower_pre(model.q1, xpi)
        q1p = q1p.squeeze(-1)
        pre += pa + pq
        dq = torch.autograd.grad(q1p.sum(), a_pi, retain_graph=True)[0]
        actor_loss = -mean(q1p)
        g_actor = torch.autograd.grad(actor_loss, ap)
        for p, g in zip(ap, g_actor):
            p.grad = g
        opts["actor"].step()
        with torch.no_grad():
            for t, c in zip(model.target_parameters(), ap + cp):
                t.copy_(torch.lerp(t, c, h["tau"]))
    else:
        g_actor = [torch.zeros_like(p) for p in ap]
        dq, a_pi, q1p, actor_loss = torch.zeros(B, A, dtype=dt), torch.zeros(B, A, dtype=dt), torch.zeros(B, dtype=dt), torch.zeros((), dtype=dt)
    n = lambda x: x.detach().numpy().astype(np.float64)
    f = lambda x: float(x.detach())
    rec = {"grad": np.concatenate([n(g).ravel() for g in list(g_actor) + list(g_critic)]), "y": n(y), "q": np.stack([n(q1), n(q2)]), "dqda": n(dq),
           "a_pi": n(a_pi), "a_next": n(a_next), "use": n(use), "stepped": stepped, "pre": np.concatenate([n(p) for p in pre], axis=1),
           "stats": {"critic_loss": f(critic_loss), "actor_loss": f(actor_loss), "q1_pi": f(mean(q1p)), "target_q": f(mean(y)), "n_use": f(n_use),
                     "actor_stepped": float(stepped), "q_abs": f(mean(q1p.abs())), "y_abs": f(mean(y.abs())),
                     "h_max": max(1.0, float(max(p.detach().abs().max() for p in pre)))}}
    if dt == torch.float64:
        pre32 = []
        with torch.no_grad():
            for seq, x in evals:
                pre32 += [n(p) for p in tower_pre(seq.float(), x.float())[1]]
        rec["pre32"] = np.concatenate(pre32, axis=1)
    return rec


def warm_state(model, h, seed=0):
    """(exp_avg, exp_avg_sq, step): an optimiser state as training holds after 4 policy_delay steps - |exp_avg| <= 1e-3, exp_avg_sq in
    [1e-5, 1e-3], aligned arrays shaped as the trained tensors"""
    rs = np.random.RandomState(907 + seed)
    shapes = [tuple(t.shape) for t in trained_of(model_tensors(model))]
    return ([PH.aligned(rs.uniform(-1e-3, 1e-3, s).astype(np.float32)) for s in shapes],
            [PH.aligned(rs.uniform(1e-5, 1e-3, s).astype(np.float32)) for s in shapes], 4 * int(h["policy_delay"]))


def torch_steps(model, batches, h, dtype, first=1, state=None):
    """the steps n_updates = first, first + 1, ... on a `dtype` copy; returns (model, opts, one record per step).  state: a warm_state to
    start the two Adams from (the critics' at its step count, the actor's at step // policy_delay; `first` counts on from it)"""
    m = copy.deepcopy(model).to(dtype)
    opts = make_opts(m, h)
    if state is not None:
        ps = trained_of(model_tensors(m))
        for i, p in enumerate(ps):
            actor = i < len(ps) // 3
            opts["actor" if actor else "critic"].state[p] = {"step": torch.tensor(float(state[2] // h["policy_delay"] if actor else state[2])),
                                                            "exp_avg": torch.from_numpy(state[0][i].copy()).to(dtype),
                                                            "exp_avg_sq": torch.from_numpy(state[1][i].copy()).to(dtype)}
        first += state[2]
    return m, opts, [torch_step(m, opts, b, h, first + i) for i, b in enumerate(batches)]


def margin(r64):
    """the ReLU margin of a case: 4 x the largest deviation of float32's hidden pre-activations from float64's on the same parameters"""
    return 4.0 * np.abs(r64["pre32"] - r64["pre"]).max()


def near_rows(model, r64, factor=1.0):
    """bool [B]: used rows with a hidden pre-activation within `factor` x the margin of 0 (ReLU only)"""
    if model.activation != "relu":
        return np.zeros(r64["use"].shape, bool)
    return (np.abs(r64["pre"]).min(1) < factor * margin(r64)) & (r64["use"] != 0)


def settle(model, b, h, n_updates, state=None):
    """rows inside a margin are taken out of the batch through `use` (masking a row moves the stepped q1 a little: repeated until no row
    is left inside); returns the batch"""
    for _ in range(12):
        r64 = torch_steps(model, [b], h, torch.float64, n_updates, state)[2][0]
        near = near_rows(model, r64, 1.5)
        if not near.any():
            return b
        use = np.ones(near.shape, np.float32) if b["use"] is None else b["use"].copy()
        use[near] = 0.0
        b = dict(b, use=use)
    return b


def reference(shape, B, seed=0, lr=None, policy_delay=1, n_updates=1):
    """the model, the warm optimiser state (m, v, step: the call is update step + n_updates), the settled batch, the float64 and float32
    torch records of that step, the yardstick and the rows the settle step took out; computed once and only read.  B = 1: the first draw seed whose row stays.  lr: in place of the default 1e-3 (0: the q1 at
    the actor step is the q1 at call start, in torch and in the build alike)"""
    key = (shape, B, seed, lr, policy_delay, n_updates)
    if key in _refs:
        return _refs[key]
    D, A = shape[0], shape[1]
    h = hyper(policy_delay=policy_delay) if lr is None else hyper(policy_delay=policy_delay, lr=lr)
    model = make_model(shape, seed)
    state = warm_state(model, h, seed)
    for s in range(seed, seed + 32):
        b0 = make_batch(D, A, B, masked=B > 1, seed=s)
        b = settle(model, b0, h, n_updates, state)
        used0 = B if b0["use"] is None else int((b0["use"] != 0).sum())
        used = B if b["use"] is None else int((b["use"] != 0).sum())
        if used >= 1 or B > 1:
            break
    lost = used0 - used
    assert used >= 1, "the case keeps no row"
    assert lost <= 0.2 * B, "the settle step took %d of %d rows: more than 20 %%" % (lost, B)
    r64, r32 = torch_steps(model, [b], h, torch.float64, n_updates, state)[2][0], torch_steps(model, [b], h, torch.float32, n_updates, state)[2][0]
    assert not near_rows(model, r64).any(), "invalid case: a used row has a hidden pre-activation inside the ReLU margin"
    sz = sizes(model)
    Y = WH.yardstick(r32["grad"], r64["grad"], sz)
    rows = r64["use"] != 0
    for k in ("y", "q", "dqda"):        # the case's one Y: torch's largest relative loss over the trained tensors and the three row blocks
        a32, a64 = (r32[k][rows], r64[k][rows]) if k == "dqda" else (r32[k], r64[k])
        if a64.size and np.abs(a64).max() > 0:
            Y = max(Y, np.abs(a32 - a64).max() / np.abs(a64).max())
    _refs[key] = dict(h=h, b=b, model=model, r64=r64, r32=r32, Y=Y, sz=sz, grp=groups(model), lost=lost,
                      n_updates=n_updates, m=state[0], v=state[1], step=state[2] + n_updates - 1)
    return _refs[key]


def check_step(out, ref, what):
    """the rule, with the case's one Y, on the gradients and on y, q and dq1/da - a row block counts as a one-tensor group:
    max|x - x64| <= 4 Y max|x64| + 2^-23 max|x64|; the stats under a bound worked out from the same Y.  Returns the figures in units of Y"""
    r64, r32, Y, model = ref["r64"], ref["r32"], ref["Y"], ref["model"]
    res = WH.rule(out["grad"], r64["grad"], Y, ref["sz"], ref["grp"])
    fig = {k: v[1] for k, v in res.items()}
    for k, (worst, in_y) in res.items():
        assert worst <= 1.0, "%s: %s gradient %.2f x its bound (%.1f Y)" % (what, k, worst, in_y)
    used = r64["use"] != 0
    for k, x, a32, a64 in (("y", out["y"], r32["y"], r64["y"]), ("q", out["q"], r32["q"], r64["q"]),
                           ("dqda", out["dqda"][used], r32["dqda"][used], r64["dqda"][used])):
        if a64.size == 0 or (k == "dqda" and not r64["stepped"]):
            continue
        big = np.abs(a64).max()
        err = np.abs(np.asarray(x, np.float64) - a64).max()
        worst, in_y = err / (4.0 * Y * big + 2.0 ** -23 * big), err / big / Y
        fig[k] = in_y
        assert worst <= 1.0, "%s: %s %.2f x its bound (%.1f Y)" % (what, k, worst, in_y)
    # the stats: a row's terms pass through fewer than 16 float32 roundings beyond the towers', the sums run in float64.  A critic's output
    # is a sum of terms whose sizes add up to at most (|W_out|_1 + |b_out|) max|h|; tanh keeps |h| <= 1, for ReLU the case's largest hidden
    # pre-activation scales it.  With d the bound of one q or y: |d critic_loss| <= 2 (mean|q1 - y| + mean|q2 - y|) 2 d <= 4 sqrt(2 critic_loss) d
    s64 = r64["stats"]
    rel = 4.0 * Y + 16 * 2.0 ** -24
    last = lambda t: t[len(t) - 1]
    hmax = s64["h_max"] if model.activation == "relu" else 1.0
    l1 = hmax * max(float((last(t).weight.abs().sum() + last(t).bias.abs().sum()).detach()) for t in (model.q1, model.q2, model.q1_target, model.q2_target))
    d = rel * (l1 + 1.0)
    tol = {"critic_loss": rel * s64["critic_loss"] + 4.0 * np.sqrt(2.0 * s64["critic_loss"]) * d, "actor_loss": rel * s64["q_abs"] + d,
           "q1_pi": rel * s64["q_abs"] + d, "target_q": rel * s64["y_abs"] + d, "n_use": 0.0, "actor_stepped": 0.0}
    for i, k in enumerate(STATS):
        assert abs(float(out["stats"][i]) - s64[k]) <= tol[k] + 2.0 ** -24 * abs(s64[k]), (what, k, out["stats"][i], s64[k], tol[k])
    assert out["stats"][6] == 0.0 and out["stats"][7] == 0.0
    return fig


def left_out(model, batches, h):
    """float64 and float32 torch over the whole steps, and the entries the parameter rule leaves out: those whose float64 gradient lies
    within the gradient rule's bound of zero at a step and is not exactly zero.  Returns (m64, m32, left [P] bool)"""
    sz, grp = sizes(model), groups(model)
    m64, _, r64 = torch_steps(model, batches, h, torch.float64)
    m32, _, r32 = torch_steps(model, batches, h, torch.float32)
    left = np.zeros(sum(sz), bool)
    for s64, s32 in zip(r64, r32):
        Yg = WH.yardstick(s32["grad"], s64["grad"], sz)
        left |= np.concatenate([(np.abs(r) <= bd) & (r != 0.0) for r, bd in zip(WH.split(s64["grad"], sz), WH.bounds(s64["grad"], Yg, sz, grp))])
    return m64, m32, left


def settled_batches(model, shape, B, n_steps, h, seed=0):
    D, A = shape[:2]
    batches = [make_batch(D, A, B, True, seed=10 * seed + s) for s in range(n_steps)]
    for i in range(n_steps):            # each step's draw settled under the float64 model as it stands at that step
        mi = torch_steps(model, batches[:i], h, torch.float64)[0]
        batches[i] = settle(mi.float(), batches[i], h, i + 1)
    return batches


def parameter_case(shape, B, n_steps, policy_delay, runner, cap, seed=0):
    """sacw_host.parameter_case for TD3: n_steps whole steps from step 0, `runner(model, batches, h)` -> (flat trained parameters, flat
    targets), the parameter rule on the entries kept.  cap: the share of a tensor that may be left out, asserted.  Returns (rule figures,
    Y, largest share left out, worst target error / bound)"""
    h = hyper(policy_delay=policy_delay)
    model = make_model(shape, seed)
    sz, grp = sizes(model), groups(model)
    batches = settled_batches(model, shape, B, n_steps, h, seed)
    m64, m32, left = left_out(model, batches, h)
    share = max(part.sum() / part.size for part in WH.split(left, sz))
    assert share <= cap, "the reference leaves out %.2f %% of a tensor's entries: more than %.2f %%" % (100 * share, 100 * cap)
    p, tg = runner(model, batches, h)
    p64, p32 = model_flat(m64), model_flat(m32)
    keep = ~left
    Y = WH.yardstick(np.where(keep, p32, p64), p64, sz)
    res = WH.rule(p, p64, Y, sz, grp, keep)
    assert np.abs(p - model_flat(model)).max() > 1e-4                     # the steps moved the parameters
    # the targets: a target entry follows its net's entry with weight tau per actor step, under the same rule on the same-shaped tensors
    t64, t32 = model_flat(m64, "targets"), model_flat(m32, "targets")
    worst_t = 0.0
    for a, a32, a64, k in zip(WH.split(np.asarray(tg, np.float64), sz), WH.split(t32, sz), WH.split(t64, sz), WH.split(keep, sz)):
        m = np.abs(a64).max()
        Yt = np.abs(np.where(k, a32, a64) - a64).max() / m
        bound = 4.0 * Yt * m + 2.0 ** -23 * np.abs(t64).max()
        worst_t = max(worst_t, np.abs(a - a64)[k].max() / bound)
    return res, Y, share, worst_t
