"""The PPO update core (csrc/xarm_ppo_core.h) on the CPU: the g++ build of the header against a torch float64 restatement of the update
(tests/ppo_host.py) - GAE, step 0's gradient under the rule of tests/a2c_host.py, the per-step stats, the parameters after a whole
update against clip_grad_norm_ + Adam, the all-masked call, out-of-range perm entries, the optimiser-state round trip, the argument
checks of the real library, the torch PPO block of train(), and an address / undefined-behaviour sanitizer run of the host core as a
stand-alone program.

The gradient rule is a2c_host.rule: per tensor max|g - g64| <= 4 Y max|g64_tensor| + 2^-23 max|g64_model|, Y what torch's float32
autograd loses against float64 on the same case.  Largest error in units of Y over these cases, host core: gradient 2.56, parameters after
a whole update 2.41 (the tests print every case's figure; DESIGN.md 22 lists them.  Y is a property of torch's CPU kernels and varies
between machines)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import a2c_host as AH
import policy_host as PH
import ppo_host as PP

SHAPES = ((1, 1), (1, 33), (5, 13))
BATCHES = (1 << 20, 64, 20)                    # N itself, 64 (5 x 13: 64 + 1, the second minibatch un-normalised), 20 (20 + 20 + 20 + 5)


# -------------------------------------------------------------------------------------------------------------------------- GAE
@pytest.mark.parametrize("lam", (0.0, 0.95, 1.0))
@pytest.mark.parametrize("T", (1, 5))
@pytest.mark.parametrize("masked", (False, True))
def test_gae_against_a_float64_recursion_from_the_same_values(T, masked, lam):
    D, A, E = 14, 4, 9
    b = PP.make_batch(D, A, T, E, 1.0, masked)
    b["done"][:] = 0.0
    b["done"][0, 0] = 1.0                      # cut at the first step
    b["done"][T // 2, 1] = 1.0                 # at a middle step
    b["done"][T - 1, 2] = 1.0                  # at the last step: the bootstrap value is cut off
    b["done"][:, 3] = 1.0                      # at every step
    model = AH.model_of(D, A, 1.0)
    w, m, v, step = PP.fresh_state(model)
    h = PP.hyper(gae_lambda=lam)
    # the host build's own float32 values: the policy's value chain
    val = PH.host_act(w, b["obs"].reshape(T * E, D), D, 0, deterministic=True)["value"].astype(np.float64).reshape(T, E)
    boot = PH.host_act(w, b["last_obs"], D, 0, deterministic=True)["value"].astype(np.float64)
    rc, out = PP.host_update(w, m, v, step, b, h, PP.make_perm(T * E, 1), T * E)
    assert rc == 0
    rew, keep = b["reward"].astype(np.float64), (b["done"] == 0).astype(np.float64)
    nv, na, adv, top = boot, np.zeros(E), np.zeros((T, E)), np.zeros(E)
    ret, a2c = boot, np.zeros((T, E))
    for k in reversed(range(T)):
        delta = rew[k] + 0.99 * keep[k] * nv - val[k]
        na = delta + 0.99 * lam * keep[k] * na
        nv = val[k]
        adv[k] = na
        top = np.maximum(top, np.abs(val[k]) + np.abs(rew[k]) + np.abs(na))
        ret = rew[k] + 0.99 * ret * keep[k]    # A2C's return (train.py's loop)
        a2c[k] = ret
    # three roundings per step
    bound = 4.0 * T * 2.0 ** -24 * top[None, :]
    assert np.all(np.abs(out["adv"] - adv) <= bound) and np.all(np.abs(out["returns"] - (adv + val)) <= bound)
    assert PH.bits(out["returns"]) == PH.bits((out["adv"] + val.astype(np.float32)).astype(np.float32))
    if lam == 1.0:
        assert np.all(np.abs(out["returns"] - a2c) <= bound)
    if lam == 0.0:                              # adv is the one-step error: an episode end leaves reward - value
        cut = b["done"] != 0
        assert np.all(np.abs(out["adv"][cut] - (rew - val)[cut]) <= 2.0 ** -23 * (np.abs(rew) + np.abs(val))[cut])
    assert np.isfinite(out["grad"]).all() and int(step[0]) == 1


# --------------------------------------------------------------------------------------------------------------------- gradient
def gradient_cases(D, A):
    shapes = SHAPES if (D, A) in ((14, 4), (96, 16)) else ((5, 13),)
    for T, E in shapes:
        for B in BATCHES:
            if B != 1 << 20 and T * E < 65:
                continue                        # one minibatch whatever the batch size
            for normalize, ent, supplied in ((1, 0.0, True), (0, 0.01, True), (1, 0.01, False), (0, 0.0, False)):
                yield T, E, B, normalize, ent, supplied


@pytest.mark.parametrize("D,A", AH.WIDTHS)
def test_first_step_gradient_and_stats_against_float64(D, A):
    worst = 0.0
    for T, E, B, normalize, ent, supplied in gradient_cases(D, A):
        r = PP.reference(D, A, T, E, B, normalize, ent, supplied)
        w, m, v, step = PP.fresh_state(AH.model_of(D, A, 1.0))
        rc, out = PP.host_update(w, m, v, step, r["b"], dict(r["h"], lr=0.0), r["perm"], B, r["old_logp"])
        assert rc == 0
        g64 = r["r64"][0]["grad"]
        ratio, in_y = AH.rule(out["grad"], g64, r["Y"], D, A)
        print("host PPO gradient D %d A %d rows %dx%d batch %d norm %d ent %g old_logp %s: Y %.2e, error %.2f Y (%s, %.1e of the model's largest entry), "
              "error / bound %.3f" % ((D, A, T, E, min(B, T * E), normalize, ent, "given" if supplied else "NULL", r["Y"], in_y) +
                                      AH.worst_tensor(out["grad"], g64, D, A) + (ratio,)))
        worst = max(worst, in_y)
        assert ratio <= 1.0, (T, E, B, normalize, ent, supplied, ratio, in_y)
        PP.check_stats(out["stats"][0], r["r64"][0], r["Y"], A)
        if supplied and T * E >= 33:
            assert 0.4 < out["stats"][0][6] < 0.9          # rows on both sides of the clip
        if not supplied:
            assert out["stats"][0][5] == 0.0 and out["stats"][0][6] == 0.0     # rho is exactly 1 at the first step
    print("host PPO gradient D %d A %d: largest error %.2f Y" % (D, A, worst))


def test_short_last_minibatch_of_one_row_is_left_unnormalised():
    D, A, T, E = 14, 4, 5, 13
    r = PP.reference(D, A, T, E, 64, 1, 0.0, True, n_steps=2)
    assert r["b"]["use"].reshape(-1)[r["perm"][0, 64]] == 1.0            # the lone row is a used one
    w, m, v, step = PP.fresh_state(AH.model_of(D, A, 1.0))
    rc, out = PP.host_update(w, m, v, step, r["b"], r["h"], r["perm"], 64, r["old_logp"])
    assert rc == 0 and out["stats"].shape == (2, 8) and out["stats"][1][4] == 1.0 and int(step[0]) == 2
    row = r["perm"][0, 64]
    assert abs(r["r64"][1]["ahat"][0] - r["prep64"][0][row]) == 0.0       # the reference took adv itself
    g64, g32 = r["r64"][1]["grad"], r["r32"][1]["grad"]
    PP.check_stats(out["stats"][1], r["r64"][1], AH.yardstick(g32, g64, D, A), A)


# ------------------------------------------------------------------------------------------------------------------- parameters
# inputs for which the union of the steps' near-zero gradient entries stays under the 1 % cap (30 x 4 with 20 or 33 rows per minibatch
# has 3 of pi_w3's 256 entries there)
@pytest.mark.parametrize("D,A,B", ((14, 4, 20), (14, 4, 33), (30, 4, 1 << 20)))
def test_whole_update_against_torch_clip_and_adam(D, A, B):
    T, E = 5, 13

    def run(r):
        w, m, v, step = PP.fresh_state(AH.model_of(D, A, 1.0))
        rc, out = PP.host_update(w, m, v, step, r["b"], r["h"], r["perm"], B, r["old_logp"])
        assert rc == 0 and int(step[0]) == out["stats"].shape[0] and np.isfinite(out["stats"]).all()
        return AH.flat_of(w)
    ratio, in_y, Y, left, S = PP.parameter_case(D, A, T, E, B, 2, run)
    print("host PPO parameters D %d A %d batch %d after %d steps: Y %.2e, error %.2f Y, error / bound %.3f, left out %d" % (D, A, B, S, Y, in_y, ratio, left))
    assert S == 2 * (-(-65 // min(B, 65))) and ratio <= 1.0


def test_all_masked_call_changes_nothing_but_the_step_count():
    D, A, T, E, B = 30, 4, 5, 13, 20
    b = PP.make_batch(D, A, T, E, 1.0)
    b["use"][:] = 0.0
    w, m, v, step = PP.fresh_state(AH.model_of(D, A, 1.0))
    before = AH.clone_weights(w)
    step[0] = 7
    rc, out = PP.host_update(w, m, v, step, b, PP.hyper(), PP.make_perm(T * E, 2), B)
    assert rc == 0 and np.all(out["grad"] == 0.0) and int(step[0]) == 7 + 8
    assert np.all(out["stats"][:, 3] == 0.0) and np.all(out["stats"][:, 4] == 1.0)
    for k in PH.NAMES:
        assert PH.bits(w[k]) == PH.bits(before[k]) and np.all(m[k] == 0.0) and np.all(v[k] == 0.0), k


def test_out_of_range_perm_entries_are_rows_with_use_zero():
    D, A, T, E, B = 14, 4, 5, 13, 20
    b, bad, b0, perm = PP.out_of_range_pair(D, A, T, E)
    h = PP.hyper()
    olp = PP.spread_old_logp(AH.model_of(D, A, 1.0), b, h)
    res = []
    for batch, pm in ((b, bad), (b0, perm)):
        w, m, v, step = PP.fresh_state(AH.model_of(D, A, 1.0))
        rc, out = PP.host_update(w, m, v, step, batch, h, pm, B, olp)
        assert rc == 0 and int(step[0]) == 4
        res.append((w, m, v, out))
    (w0, m0, v0, o0), (w1, m1, v1, o1) = res
    assert all(PH.bits(o0[k]) == PH.bits(o1[k]) for k in ("adv", "returns", "grad", "stats"))
    assert o0["stats"][:, 4].sum() == b0["use"].sum() < b["use"].sum()
    for k in PH.NAMES:
        assert PH.bits(w0[k]) == PH.bits(w1[k]) and PH.bits(m0[k]) == PH.bits(m1[k]) and PH.bits(v0[k]) == PH.bits(v1[k]), k


# ------------------------------------------------------------------------------------------------------------- optimiser state
def torch_calls(model, batches, h, dtype):
    """one single-step update (one epoch, one minibatch of all rows, old_logp from the call's own weights) per batch with one Adam"""
    import copy
    m = copy.deepcopy(model).to(dtype)
    opt = torch.optim.Adam(m.parameters(), lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
    for b in batches:
        N = b["reward"].size
        loss, _ = PP.torch_step_loss(m, b, h, PP.torch_prepare(m, b, h), torch.arange(N))
        opt.zero_grad(set_to_none=True)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), h["max_grad_norm"])
        opt.step()
    return m, opt


def test_optimizer_state_round_trip():
    """an Adam that has taken two steps hands its state over, the host build takes the third step, and a fresh Adam continues from the
    exported state with the fourth: as torch alone"""
    from gym_xarm_amd.device_ppo import export_adam, load_adam
    from gym_xarm_amd.device_a2c import module_params
    D, A, T, E = 14, 4, 5, 13
    N = T * E
    h = PP.hyper()
    batches = [PP.make_batch(D, A, T, E, 1.0, seed=s) for s in range(4)]
    ident = np.arange(N, dtype=np.int32)[None, :].copy()
    model = PH.case(D, 0, A, 1.0)["model"]
    m2, opt2 = torch_calls(model, batches[:2], h, torch.float32)
    m3, opt3 = torch_calls(model, batches[:3], h, torch.float32)
    m4, _ = torch_calls(model, batches, h, torch.float32)
    pm = module_params(m2)
    ea, es, st = [torch.zeros_like(p) for p in pm], [torch.zeros_like(p) for p in pm], torch.zeros(1, dtype=torch.int64)
    load_adam(ea, es, st, opt2, pm)
    assert int(st[0]) == 2
    for x, y, p in zip(ea, es, pm):
        assert torch.equal(x, opt2.state[p]["exp_avg"]) and torch.equal(y, opt2.state[p]["exp_avg_sq"]) and x.data_ptr() != opt2.state[p]["exp_avg"].data_ptr()
    w = PH.weights_of(m2)
    mm, vv = ({k: PH.aligned(t.numpy()) for k, t in zip(PH.NAMES, xs)} for xs in (ea, es))
    step = st.numpy().copy()
    rc, _ = PP.host_update(w, mm, vv, step, batches[2], h, ident, N)
    assert rc == 0 and int(step[0]) == 3
    # the third step's state against torch's own float32 one.  Both gradients lie within (4 + 1) Y_g of float64's relative to the
    # tensor's largest entry, a square doubles a relative error, and the clip's norm adds as much again: 16 Y_g, plus the roundings of
    # the state's own update (test_a2c_host.py's bound; exp_avg is linear in the gradient and obeys it a fortiori)
    _, _, r64, _ = PP.torch_update(m2, batches[2], h, ident, N, torch.float64)
    _, _, r32, _ = PP.torch_update(m2, batches[2], h, ident, N, torch.float32)
    Yg = AH.yardstick(r32[0]["grad"], r64[0]["grad"], D, A)
    for k, p in zip(PH.NAMES, module_params(m3)):
        for mine, name in ((mm, "exp_avg"), (vv, "exp_avg_sq")):
            ref = opt3.state[p][name].numpy().astype(np.float64)
            assert np.abs(mine[k] - ref).max() <= (16.0 * Yg + 2.0 ** -22) * np.abs(ref).max(), (k, name)
    # export into a fresh optimiser on a module that holds the host build's parameters, and take the fourth step with torch
    m = AH.model_of(D, A, 1.0)
    with torch.no_grad():
        for k, p in zip(PH.NAMES, module_params(m)):
            p.copy_(torch.from_numpy(w[k]))
    opt = torch.optim.Adam(m.parameters(), lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
    export_adam([torch.from_numpy(mm[k]) for k in PH.NAMES], [torch.from_numpy(vv[k]) for k in PH.NAMES], torch.from_numpy(step), opt, module_params(m))
    for k, p in zip(PH.NAMES, module_params(m)):
        assert PH.bits(opt.state[p]["exp_avg"].numpy()) == PH.bits(mm[k]) and PH.bits(opt.state[p]["exp_avg_sq"].numpy()) == PH.bits(vv[k])
        assert float(opt.state[p]["step"]) == 3.0
    ba, bs, bt = [torch.zeros_like(p) for p in pm], [torch.zeros_like(p) for p in pm], torch.zeros(1, dtype=torch.int64)
    load_adam(ba, bs, bt, opt, module_params(m))
    assert int(bt[0]) == 3
    for k, x, y in zip(PH.NAMES, ba, bs):
        assert PH.bits(x.numpy()) == PH.bits(mm[k]) and PH.bits(y.numpy()) == PH.bits(vv[k])          # both directions, bit for bit
    loss, _ = PP.torch_step_loss(m, batches[3], h, PP.torch_prepare(m, batches[3], h), torch.arange(N))
    opt.zero_grad(set_to_none=True)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(m.parameters(), h["max_grad_norm"])
    opt.step()
    # the fourth step moves an entry by about lr: continuing from the handed-over state lands on torch's own fourth step
    for p, q in zip(module_params(m), module_params(m4)):
        assert float(opt.state[p]["step"]) == 4.0 and (p - q).abs().max() <= 0.05 * h["lr"]
    with pytest.raises(ValueError, match="amsgrad"):
        load_adam(ba, bs, bt, torch.optim.Adam(m.parameters(), amsgrad=True), module_params(m))
    with pytest.raises(ValueError, match="weight decay"):
        export_adam(ba, bs, bt, torch.optim.Adam(m.parameters(), weight_decay=0.1), module_params(m))


def test_device_class_refuses_a_cpu_model():
    from gym_xarm_amd.device_ppo import DevicePPO
    with pytest.raises(ValueError, match="torch PPO block of train.py"):
        DevicePPO(AH.model_of(14, 4, 1.0), num_envs=8)


# ------------------------------------------------------------------------------------------------------------- argument checks
def test_invalid_arguments_are_refused_by_the_library():
    """every XARM_E_INVALID case of xarm_ppo_update through libxarm_hip.so itself (the checks come before any launch, so they run
    without a GPU) and through the host build, which shares the checks"""
    from gym_xarm_amd import _native
    L = _native.load()
    D, A, T, E = 14, 4, 5, 13
    N = T * E
    b = PP.make_batch(D, A, T, E, 1.0)
    w, m, v, step = PP.fresh_state(AH.model_of(D, A, 1.0))
    perm = PP.make_perm(N, 2)
    work = PH.aligned(np.zeros(8, np.float32))
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(layout=None, params=None, null=(), misalign=None, struct_null=(), work_ptr="ok"):
        layout = layout or _native.XarmPPOLayout(E, T, D, A, 64, 2, 20)
        params = params or PP.abi_params(PP.hyper())
        ptrs = {"w": {k: w[k].ctypes.data for k in PH.NAMES}, "m": {k: m[k].ctypes.data for k in PH.NAMES}, "v": {k: v[k].ctypes.data for k in PH.NAMES}}
        for k in null:
            if "." in k:
                ptrs[k[0]][k[2:]] = None
        if misalign:
            ptrs["w"][misalign] += 4
        S = {s: _native.XarmPolicyWeights(*[ptrs[s][k] for k in PH.NAMES]) for s in "wmv"}
        data = {k: (None if k in null else P(b[k])) for k in ("obs", "action", "reward", "done", "use", "last_obs")}
        wk = {"ok": P(work), "null": None, "odd": C.c_void_p(work.ctypes.data + 4)}[work_ptr]
        args = [None if "layout" in struct_null else C.byref(layout), None if "params" in struct_null else C.byref(params)] + \
               [None if s in struct_null else C.byref(S[s]) for s in "wmv"] + \
               [None if "step" in null else P(step), data["obs"], data["action"], data["reward"], data["done"], data["use"], data["last_obs"], None,
                None if "perm" in null else P(perm), wk, None, None, None, None]
        return L.xarm_ppo_update(*args, None), PP.lib().ph_update(*args, None)

    def refused(**kw):
        rc, rh = call(**kw)
        return rc == -1 and rh == -1 and b"xarm_ppo_update" in L.xarm_last_error(None)

    lay = lambda **kw: _native.XarmPPOLayout(**dict(dict(num_envs=E, n_steps=T, obs_dim=D, act_dim=A, hidden=64, n_epochs=2, batch_size=20), **kw))
    par = lambda **kw: PP.abi_params(PP.hyper(**kw))
    for s in ("layout", "params", "w", "m", "v"):
        assert refused(struct_null=(s,)), s
    # everything xarm_a2c_update refuses
    for kw in (dict(num_envs=-1), dict(n_steps=0), dict(n_steps=-3), dict(obs_dim=0), dict(obs_dim=97), dict(act_dim=0), dict(act_dim=17), dict(hidden=32),
               dict(num_envs=1 << 29, n_steps=4, batch_size=1 << 30), dict(num_envs=(1 << 31) - 1, n_steps=2, batch_size=1 << 30),
               # and the PPO layout's own
               dict(n_epochs=0), dict(n_epochs=-1), dict(batch_size=0), dict(batch_size=-5), dict(n_epochs=64, batch_size=1), dict(n_epochs=4097, batch_size=N)):
        assert refused(layout=lay(**kw)), kw
    assert call(layout=lay(n_epochs=4096, batch_size=N), work_ptr="null")[0] == -1 and b"workspace" in L.xarm_last_error(None)   # 4096 steps pass the layout check
    for kw in (dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(lr=-1e-3), dict(eps=0.0), dict(eps=-1e-5),
               dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(vf_coef=float("inf")), dict(ent_coef=float("nan")),
               dict(gae_lambda=-0.1), dict(gae_lambda=1.01), dict(gae_lambda=float("nan")), dict(clip_range=0.0), dict(clip_range=-0.2),
               dict(clip_range=float("inf")), dict(clip_range=float("nan")), dict(beta1=-0.1), dict(beta1=1.0), dict(beta2=1.0), dict(beta2=-0.5),
               dict(beta2=float("nan"))):
        assert refused(params=par(**kw)), kw
    for k in PH.NAMES:
        for s in "wmv":
            assert refused(null=(s + "." + k,)), (s, k)
    for k in ("pi_b1", "pi_w2", "pi_b2", "pi_w3", "vf_b1", "vf_w2", "vf_b2", "vf_w3"):
        assert refused(misalign=k), k
    for k in ("obs", "action", "reward", "done", "last_obs", "step", "perm"):
        assert refused(null=(k,)), k
    assert refused(work_ptr="null") and refused(work_ptr="odd")
    # num_envs == 0 is a no-op that returns OK whatever the pointers are
    assert call(layout=lay(num_envs=0), null=("obs", "action", "reward", "done", "last_obs", "step", "perm"), work_ptr="null") == (0, 0)
    # the workspace size: refused for an unusable layout, positive and 16-byte granular otherwise, and what the host build states
    n = C.c_int64(-5)
    assert L.xarm_ppo_workspace_bytes(C.byref(lay(n_epochs=0)), C.byref(n)) == -1 and L.xarm_ppo_workspace_bytes(C.byref(lay()), None) == -1
    assert L.xarm_ppo_workspace_bytes(None, C.byref(n)) == -1
    assert L.xarm_ppo_workspace_bytes(C.byref(lay()), C.byref(n)) == 0 and n.value > 0 and n.value % 16 == 0
    assert n.value == PP.lib().ph_workspace_bytes(C.byref(lay()))
    assert PP.geometry(T, E, D, A, 2, 20)[4:] == [20, 4, 8, 4 + 3 * 8]


# ----------------------------------------------------------------------------------------------------------------------- driver
@pytest.mark.parametrize("lazy", (False, True))
def test_train_runs_the_torch_ppo_block_on_the_scripted_env(lazy):
    """the CPU stand-in env of tests/test_train_driver.py: 3 updates of 8 x 16 rows, 2 epochs x 3 minibatches (48 + 48 + 32)"""
    from test_train_driver import ScriptedEnv
    from gym_xarm_amd.train import ActorCritic, train
    model, venv, hist = train(env_id="Scripted-v0", env=ScriptedEnv(16, lazy=lazy), updates=3, algo="ppo", n_steps=8, n_epochs=2, batch_size=48,
                              quiet=True, log_every=3, auto_reset="lazy" if lazy else True)
    assert len(hist) == 1 and hist[0]["env_steps"] == 3 * 8 * 16 and all(np.isfinite(x) for x in hist[0].values())
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    torch.manual_seed(0)
    start = ActorCritic(venv.dim, 2)
    moved = max(float((p - q).detach().abs().max()) for p, q in zip(model.parameters(), start.parameters()))
    assert 1e-4 < moved <= 18 * 3e-4 * 1.5              # 18 Adam steps of about lr each
    # the defaults of algo="ppo": 16-step rollouts
    _, _, hist = train(env_id="Scripted-v0", env=ScriptedEnv(16), updates=1, algo="ppo", quiet=True, log_every=1)
    assert hist[0]["env_steps"] == 16 * 16
    with pytest.raises(ValueError, match="algo"):
        train(env_id="Scripted-v0", env=ScriptedEnv(16), updates=1, algo="trpo", quiet=True)


# ---------------------------------------------------------------------------------------------------------------------- sanitizers
def _have_sanitizers():
    """libasan / libubsan are installed and a sanitized program starts in this environment"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "san_probe")
        return subprocess.run(["g++", "-x", "c++", "-", "-fsanitize=address,undefined", "-o", exe], input=b"int main(){return 0;}",
                              capture_output=True).returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason="libasan/libubsan not available")
def test_host_core_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """updates over the row counts, widths and batch sizes of these tests through the host core as a stand-alone program (its own main,
    never loaded into python)"""
    exe = str(tmp_path / "ppo_main_san")
    src = os.path.join(PP.DIR, "ppo_main.cpp")
    subprocess.check_call(["g++", "-g"] + PH.gxx_flags() + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                            "-fno-omit-frame-pointer", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ppo_main ok" in r.stdout and "ERROR" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
