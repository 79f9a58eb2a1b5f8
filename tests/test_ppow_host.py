"""CPU-side tests of the wide on-policy path: ActorCritic(net_arch, activation), the torch block and the checkpoint on it,
the g++ host build of csrc/xarm_acw_core.h and csrc/xarm_ppow_core.h (tests/hostbuild_ppow) against train.py's own PPO functions in
float64 under the rule of tests/ppow_host.py, the argument checks of xarm_acw_* / xarm_ppow_* through libxarm_hip.so itself (they come
before any launch), the device classes' shape checks, the driver and the sanitizer run."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest
import torch

import policy_host as PH
import ppo_host as PP
import ppow_host as W

# sha256 over the state_dict's tensors of ActorCritic(14, 4) built under torch.manual_seed(1234) by the commit before net_arch existed
PARENT_SHA = "1eb2478d3ae064128192064b9a31ff05a777b71779552a09eea82fa6ef442f88"
PARENT_KEYS = ["log_std", "pi.0.weight", "pi.0.bias", "pi.2.weight", "pi.2.bias", "pi.4.weight", "pi.4.bias",
               "vf.0.weight", "vf.0.bias", "vf.2.weight", "vf.2.bias", "vf.4.weight", "vf.4.bias"]


# ------------------------------------------------------------------------------------------------------------------- the module
def test_default_module_is_the_64_64_tanh_module_bit_for_bit():
    from gym_xarm_amd.train import ActorCritic
    torch.manual_seed(1234)
    m = ActorCritic(14, 4)
    sd = m.state_dict()
    assert list(sd.keys()) == PARENT_KEYS and m.net_arch == (64, 64) and m.activation == "tanh"
    assert hashlib.sha256(b"".join(v.numpy().tobytes() for v in sd.values())).hexdigest() == PARENT_SHA
    assert [type(x).__name__ for x in m.pi] == ["Linear", "Tanh", "Linear", "Tanh", "Linear"]
    with pytest.raises(ValueError):
        ActorCritic(14, 4, activation="gelu")
    with pytest.raises(ValueError):
        ActorCritic(14, 4, net_arch=())


def test_wide_relu_module_and_the_torch_learner():
    from gym_xarm_amd.train import ActorCritic, TorchPPO
    m = ActorCritic(14, 4, net_arch=(256, 256, 256), activation="relu")
    assert [tuple(p.shape) for p in m.pi.parameters()] == [(256, 14), (256,), (256, 256), (256,), (256, 256), (256,), (4, 256), (4,)]
    assert [tuple(p.shape) for p in m.vf.parameters()] == [(256, 14), (256,), (256, 256), (256,), (256, 256), (256,), (1, 256), (1,)]
    assert [type(x).__name__ for x in m.vf] == ["Linear", "ReLU"] * 3 + ["Linear"]
    learner = TorchPPO(m, num_envs=6, n_steps=3, n_epochs=1, batch_size=9)
    assert learner.buffers["action"].shape == (3, 6, 4) and learner.buffers["obs"].shape == (3, 6, 14)
    before = [p.detach().clone() for p in m.parameters()]
    learner.buffers["obs"].normal_()
    learner.buffers["reward"].normal_()
    learner.update(torch.randn(6, 14))
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters()) and any(not torch.equal(p, q) for p, q in zip(m.parameters(), before))


def test_checkpoint_round_trip_rebuilds_the_shape(tmp_path):
    from gym_xarm_amd import train as TR

    class Stats:
        def state_dict(self):
            return {"obs_mean": torch.arange(3.0)}
    for arch, act in (((256, 256, 256), "relu"), ((64, 64), "tanh"), ((128, 128), "tanh")):
        m = TR.ActorCritic(9, 3, arch, act)
        path = str(tmp_path / ("m%d.safetensors" % len(arch)))
        TR.save_model(path, m, Stats())
        back, vn = TR.load_checkpoint(path)
        assert back.net_arch == arch and back.activation == act and torch.equal(vn["obs_mean"], torch.arange(3.0))
        assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), m.state_dict().values()))
    # a file without the metadata is the 64-64 tanh shape
    from safetensors.torch import save_file
    m = TR.ActorCritic(9, 3)
    save_file({"policy." + k: v.contiguous() for k, v in m.state_dict().items()}, str(tmp_path / "old.safetensors"))
    back, vn = TR.load_checkpoint(str(tmp_path / "old.safetensors"))
    assert back.net_arch == (64, 64) and vn == {} and torch.equal(back.pi[4].weight, m.pi[4].weight)


def test_device_classes_select_or_refuse_by_shape():
    from gym_xarm_amd.device_a2c import DeviceA2C
    from gym_xarm_amd.device_policy import DevicePolicy
    from gym_xarm_amd.device_ppo import DevicePPO
    from gym_xarm_amd.train import ActorCritic
    assert DevicePolicy(ActorCritic(14, 4)).backend == "tile64" and DevicePolicy(ActorCritic(14, 4), wide=True).backend == "wide"
    assert DevicePolicy(ActorCritic(14, 4, (256, 256, 256), "relu")).backend == "wide"
    assert DevicePolicy(ActorCritic(14, 4, (64, 64), "relu")).backend == "wide" and DevicePolicy(ActorCritic(14, 4, (64, 64, 64))).backend == "wide"
    for arch, act in (((256, 128), "tanh"), ((320, 320), "tanh"), ((64,), "tanh"), ((64, 64, 64, 64), "relu"), ((100, 100), "relu")):
        with pytest.raises(ValueError, match="64, 128, 192 or 256.*ActorCritic.dist"):
            DevicePolicy(ActorCritic(14, 4, arch, act))
        with pytest.raises(ValueError, match="64, 128, 192 or 256.*ppo_update"):
            DevicePPO(ActorCritic(14, 4, arch, act), num_envs=8)
    with pytest.raises(ValueError, match="64-64"):
        DevicePolicy(ActorCritic(14, 4, (128, 128)), wide=False)
    for arch, act in (((128, 128), "tanh"), ((64, 64), "relu"), ((64, 64, 64), "tanh")):
        with pytest.raises(ValueError, match="64-64.*a2c_update"):
            DeviceA2C(ActorCritic(14, 4, arch, act), num_envs=8)
    with pytest.raises(ValueError, match="torch PPO block of train.py"):             # a supported shape on the CPU: no host path
        DevicePPO(ActorCritic(14, 4, (128, 128), "relu"), num_envs=8)


# ------------------------------------------------------------------------------------------------------------------- the update
def host_first_step(shape, T, E, B, normalize, ent, supplied, masked=True):
    r = W.reference(shape, T, E, B, normalize, ent, supplied, masked=masked)
    model = W.model_of(shape)
    w, m, v, step = W.fresh_state(model)
    rc, out = W.host_update(w, m, v, step, r["b"], dict(r["h"], lr=0.0), r["perm"], B, shape, r["old_logp"])
    assert rc == 0 and int(step[0]) == PP.steps_of(T * E, 1, B)
    assert all(PH.bits(a) == PH.bits(b) for a, b in zip(w, W.weights_of(model)))           # lr = 0 leaves the parameters alone
    return r, out


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_first_step_gradient_stats_and_advantages_against_float64(case):
    shape, T, E = case
    worst = 0.0
    for normalize, ent, supplied, masked in ((1, 0.01, True, True), (1, 0.0, False, True), (0, 0.0, True, False)):
        r, out = host_first_step(shape, T, E, W.BATCH, normalize, ent, supplied, masked)
        ratio, in_y = W.rule(out["grad"], r["r64"][0]["grad"], r["Y"], r["sizes"])
        print("wide host PPO gradient %s norm %d ent %g old_logp %s: Y %.2e, error %.2f Y, error / bound %.3f, margin %.1e settled out %d"
              % (W.case_id(case), normalize, ent, "given" if supplied else "NULL", r["Y"], in_y, ratio, r["margin"], r["taken"]))
        assert ratio <= 1.0
        worst = max(worst, in_y)
        PP.check_stats(out["stats"][0], r["r64"][0], r["Y"], shape[1])
        if supplied and T * E >= 13:
            assert out["stats"][0][6] > 0.0                              # the spread old_logp clips rows
        if not supplied:
            assert out["stats"][0][5] == 0.0 and out["stats"][0][6] == 0.0   # every ratio of step 0 is exactly 1
        # adv and ret: float32 chains of D, then hidden terms per layer, then three roundings per step (DESIGN.md 22's bound for this shape)
        adv64, ret64 = r["prep64"][0].reshape(T, E), r["prep64"][1].reshape(T, E)
        top = max(np.abs(ret64).max(), np.abs(adv64).max())
        bound = (shape[0] + shape[2] * shape[3] + 4 * T) * 2.0 ** -24 * T * top
        assert np.abs(out["returns"] - ret64).max() <= bound and np.abs(out["adv"] - adv64).max() <= bound
    print("wide host PPO gradient %s: largest error %.2f Y" % (W.case_id(case), worst))


def test_geometry_and_launch_count():
    geo = W.geometry(5, 13, W.SHAPE_REF, 2, 33)
    assert (geo["B"], geo["M"], geo["S"], geo["chunks"], geo["ranges"]) == (33, 2, 4, 3, 1) and geo["launches"] == 3 * 4 + 2 + 4 * 12
    assert geo["P"] == sum(W.sizes(W.model_of(W.SHAPE_REF))) and geo["NT"] == 17
    geo = W.geometry(1, 4097, W.SHAPE_A, 1, 4097)
    assert geo["ranges"] == 16 and geo["rows"][:3] == [0, 256, 512] and geo["rows"][16] == 4097 and geo["launches"] == 2 * 3 + 2 + 10
    assert W.geometry(16, 64, W.SHAPE_A, 4, 256)["chunks"] == 4 + 1 and W.geometry(2, 100, W.SHAPE_A, 1, 30)["chunks"] == 7 + 4


def test_all_masked_call_changes_nothing_but_the_step_count():
    shape, T, E = W.SHAPE_REF, 5, 13
    b = W.make_batch(shape, T, E)
    b["use"][:] = 0.0
    model = W.model_of(shape)
    w, m, v, step = W.fresh_state(model)
    step[0] = 7
    rc, out = W.host_update(w, m, v, step, b, PP.hyper(), PP.make_perm(T * E, 2), 20, shape)
    assert rc == 0 and int(step[0]) == 7 + 8 and (out["grad"] == 0).all() and (out["stats"][:, 3] == 0).all() and (out["stats"][:, 4] == 1).all()
    for a, a0, mm, vv in zip(w, W.weights_of(model), m, v):
        assert PH.bits(a) == PH.bits(a0) and (mm == 0).all() and (vv == 0).all()


def test_out_of_range_perm_entries_are_rows_with_use_zero():
    shape, T, E, B = W.SHAPE_A, 5, 13, 20
    N = T * E
    b = W.make_batch(shape, T, E)
    perm = PP.make_perm(N, 1)
    bad = perm.copy()
    pos = np.random.RandomState(5).permutation(N)[:max(N // 10, 2)]
    bad[0, pos[0::2]] = -1
    bad[0, pos[1::2]] = N
    b0 = dict(b, use=b["use"].copy())
    b0["use"].reshape(-1)[perm[0, pos]] = 0.0
    res = []
    for batch, pm in ((b, bad), (b0, perm)):
        w, m, v, step = W.fresh_state(W.model_of(shape))
        rc, out = W.host_update(w, m, v, step, batch, PP.hyper(), pm, B, shape)
        assert rc == 0 and int(step[0]) == 4
        res.append(w + m + v + [out["grad"], out["stats"], out["adv"], out["returns"]])
    for x, y in zip(*res):
        assert np.isfinite(x).all() and PH.bits(x) == PH.bits(y)


def parameter_case(shape, T, E, B, n_epochs, cap):
    """2 x 2 optimiser steps of the host build against torch's float64 update under DESIGN.md 21's parameter rule; entries whose float64
    gradient lies within the gradient bound of zero at any step are left out, at most `cap` of a tensor"""
    r = W.reference(shape, T, E, B, 1, 0.0, True, n_epochs=n_epochs, n_steps=1 << 20)
    model, sz = W.model_of(shape), r["sizes"]
    m64, _, _, _ = W.torch_update(model, r["b"], r["h"], r["perm"], B, torch.float64, r["old_logp"])
    m32, _, _, _ = W.torch_update(model, r["b"], r["h"], r["perm"], B, torch.float32, r["old_logp"])
    left_out = np.zeros(sum(sz), bool)
    for s64, s32 in zip(r["r64"], r["r32"]):
        left_out |= W.sensitive(s64["grad"], W.yardstick(s32["grad"], s64["grad"], sz), sz)
    share = max(part.sum() / part.size for part in W.split(left_out, sz))
    assert share <= cap, "%.2f %% of a tensor's entries have a float64 gradient at zero" % (100 * share)
    w, m, v, step = W.fresh_state(model)
    rc, out = W.host_update(w, m, v, step, r["b"], r["h"], r["perm"], B, shape, r["old_logp"])
    assert rc == 0 and int(step[0]) == len(r["r64"])
    p, p64, p32 = W.flat_of(w), W.flat_of(W.weights_of(m64)), W.flat_of(W.weights_of(m32))
    p64 = np.concatenate([t.detach().numpy().ravel() for t in W.tensors_of(m64)])
    keep = ~left_out
    Y = W.yardstick(np.where(keep, p32, p64), p64, sz)
    ratio, in_y = W.rule(p, p64, Y, sz, keep)
    assert np.abs(p - W.flat_of(W.weights_of(model))).max() > 1e-4
    print("wide host PPO parameters %s after %d steps: Y %.2e, error %.2f Y, error / bound %.3f, left out %d (largest share of a tensor %.3f %%)"
          % (W.case_id((shape, T, E)), len(r["r64"]), Y, in_y, ratio, int(left_out.sum()), 100 * share))
    return ratio


# the share of a tensor that DESIGN.md 21's parameter rule may leave out: 1 % for every case.  At (30, 4, 256, 3, relu) the float64 / float32
# torch pair alone leaves out 0.27 - 0.48 % of a tensor over four draws of the batch, so that case stays inside 1 % too; its
# cap is twice the largest draw.
PARAMETER_CASES = ((W.SHAPE_A, 0.01), ((30, 4, 256, 2, "tanh"), 0.01), (W.SHAPE_REF, 0.0096))


@pytest.mark.parametrize("shape,cap", PARAMETER_CASES, ids=lambda s: "D%d-A%d-%dx%d-%s" % s if isinstance(s, tuple) else str(s))
def test_parameters_after_two_epochs_of_two_minibatches(shape, cap):
    assert parameter_case(shape, 5, 13, W.BATCH, 2, cap) <= 1.0


def test_optimizer_state_round_trip_on_a_wide_module():
    """device_ppo.load_adam / export_adam with a torch.optim.Adam that has taken two steps, on the wide module's 17 tensors"""
    from gym_xarm_amd.device_ppo import export_adam, load_adam
    model = W.model_of(W.SHAPE_ODD)
    params = W.tensors_of(model)
    opt = torch.optim.Adam(model.parameters(), lr=3e-4, eps=1e-5)
    for _ in range(2):
        opt.zero_grad()
        (model.pi(torch.randn(8, 29)).sum() + model.value(torch.randn(8, 29)).sum() + model.log_std.sum()).backward()
        opt.step()
    m, v, step = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params], torch.zeros(1, dtype=torch.int64)
    load_adam(m, v, step, opt, params)
    assert int(step) == 2 and len(m) == 17 and all(torch.equal(a, opt.state[p]["exp_avg"]) and torch.equal(b, opt.state[p]["exp_avg_sq"]) for a, b, p in zip(m, v, params))
    fresh = torch.optim.Adam(model.parameters(), lr=3e-4, eps=1e-5)
    export_adam(m, v, step, fresh, params)
    assert all(int(fresh.state[p]["step"]) == 2 and torch.equal(fresh.state[p]["exp_avg"], a) for a, p in zip(m, params))


# ------------------------------------------------------------------------------------------------------------- argument checks
def test_invalid_arguments_are_refused_by_the_library():
    """every XARM_E_INVALID case of xarm_ppow_update and xarm_acw_act through libxarm_hip.so itself (the checks come before any launch, so
    they run without a GPU) and through the host build, which shares the checks"""
    from gym_xarm_amd import _native
    L = _native.load()
    assert C.sizeof(_native.XarmACWLayout) == 40 and C.sizeof(_native.XarmPPOWLayout) == 36 and C.sizeof(_native.XarmACWWeights) == 17 * 8
    shape, T, E = W.SHAPE_REF, 5, 13
    D, A, H, NL, _ = shape
    N = T * E
    b = W.make_batch(shape, T, E)
    w, m, v, step = W.fresh_state(W.model_of(shape))
    perm = PP.make_perm(N, 2)
    work = PH.aligned(np.zeros(8, np.float32))
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    NT = len(w)

    def weights(arrs, null=None, misalign=None):
        ptr = [a.ctypes.data for a in arrs]
        s = _native.XarmACWWeights()
        for i in range(NT):
            x = None if i == null else ptr[i] + (4 if i == misalign else 0)
            if i == NT - 1:
                s.log_std = x
            else:
                (s.pi if i < 8 else s.vf)[i % 8] = x
        return s

    def call(layout=None, params=None, null=(), wnull=None, misalign=None, struct_null=(), work_ptr="ok"):
        layout = layout or W.abi_layout(T, E, shape, 2, 20)
        params = params or PP.abi_params(PP.hyper())
        S = {"w": weights(w, wnull[1] if wnull and wnull[0] == "w" else None, misalign), "m": weights(m, wnull[1] if wnull and wnull[0] == "m" else None),
             "v": weights(v, wnull[1] if wnull and wnull[0] == "v" else None)}
        data = {k: (None if k in null else P(b[k])) for k in ("obs", "action", "reward", "done", "use", "last_obs")}
        wk = {"ok": P(work), "null": None, "odd": C.c_void_p(work.ctypes.data + 4)}[work_ptr]
        args = [None if "layout" in struct_null else C.byref(layout), None if "params" in struct_null else C.byref(params)] + \
               [None if s in struct_null else C.byref(S[s]) for s in "wmv"] + \
               [None if "step" in null else P(step), data["obs"], data["action"], data["reward"], data["done"], data["use"], data["last_obs"], None,
                None if "perm" in null else P(perm), wk, None, None, None, None]
        return L.xarm_ppow_update(*args, None), W.lib().pwh_update(*args)

    def refused(**kw):
        rc, rh = call(**kw)
        return rc == -1 and rh == -1 and b"xarm_ppow_update" in L.xarm_last_error(None)

    lay = lambda **kw: _native.XarmPPOWLayout(**dict(dict(num_envs=E, n_steps=T, obs_dim=D, act_dim=A, hidden=H, n_hidden=NL, activation=1, n_epochs=2, batch_size=20), **kw))
    par = lambda **kw: PP.abi_params(PP.hyper(**kw))
    for s in ("layout", "params", "w", "m", "v"):
        assert refused(struct_null=(s,)), s
    for kw in (dict(hidden=32), dict(hidden=96), dict(hidden=320), dict(hidden=0), dict(n_hidden=1), dict(n_hidden=4), dict(activation=2), dict(activation=-1),
               dict(num_envs=-1), dict(n_steps=0), dict(obs_dim=0), dict(obs_dim=97), dict(act_dim=0), dict(act_dim=17),
               dict(num_envs=1 << 29, n_steps=4, batch_size=1 << 30), dict(n_epochs=0), dict(batch_size=0), dict(batch_size=-5), dict(n_epochs=64, batch_size=1),
               dict(n_epochs=4097, batch_size=N)):
        assert refused(layout=lay(**kw)), kw
    for kw in (dict(gamma=-0.1), dict(gamma=float("nan")), dict(lr=-1e-3), dict(eps=0.0), dict(max_grad_norm=0.0), dict(vf_coef=float("inf")),
               dict(ent_coef=float("nan")), dict(gae_lambda=1.01), dict(clip_range=0.0), dict(clip_range=float("nan")), dict(beta1=1.0), dict(beta2=-0.5)):
        assert refused(params=par(**kw)), kw
    for i in range(NT):
        for s in "wmv":
            assert refused(wnull=(s, i)), (s, i)
    for i in list(range(1, 7)) + list(range(9, 15)):                       # b1 .. W_out of either tower
        assert refused(misalign=i), i
    for k in ("obs", "action", "reward", "done", "last_obs", "step", "perm"):
        assert refused(null=(k,)), k
    assert refused(work_ptr="null") and refused(work_ptr="odd")
    assert call(layout=lay(num_envs=0), null=("obs", "action", "reward", "done", "last_obs", "step", "perm"), work_ptr="null") == (0, 0)
    n = C.c_int64(-5)
    assert L.xarm_ppow_workspace_bytes(C.byref(lay(n_hidden=5)), C.byref(n)) == -1 and L.xarm_ppow_workspace_bytes(C.byref(lay()), None) == -1
    assert L.xarm_ppow_workspace_bytes(None, C.byref(n)) == -1
    assert L.xarm_ppow_workspace_bytes(C.byref(lay()), C.byref(n)) == 0 and n.value > 0 and n.value % 16 == 0
    assert n.value == W.lib().pwh_workspace_bytes(C.byref(lay()))

    # ---- xarm_acw_act
    rows = PH.aligned(np.zeros((E, D), np.float32))
    calls = np.zeros(1, np.int64)
    awork = PH.aligned(np.zeros(8, np.float32))

    def act(layout=None, params=None, wnull=None, misalign=None, struct_null=(), null=(), work_ptr="ok", value=True, det=0):
        layout = layout or W.act_layout(E, shape)
        params = params or _native.XarmPolicyParams(0, 10.0, 1e-8, det)
        ws = weights(w, wnull, misalign)
        wk = {"ok": P(awork), "null": None, "odd": C.c_void_p(awork.ctypes.data + 4)}[work_ptr]
        args = [None if "layout" in struct_null else C.byref(layout), None if "params" in struct_null else C.byref(params), None if "w" in struct_null else C.byref(ws),
                None, None if "calls" in null else P(calls), None if "obs" in null else P(rows),
                None if "ag" in null else P(rows), None if "dg" in null else P(rows), wk, None, None, None, P(rows) if value else None]
        return L.xarm_acw_act(*args, None), W.lib().pwh_act(*args)

    def act_refused(**kw):
        rc, rh = act(**kw)
        return rc == -1 and rh == -1 and b"xarm_acw_act" in L.xarm_last_error(None)

    alay = lambda **kw: _native.XarmACWLayout(**dict(dict(num_rows=E, obs_dim=D, goal_dim=0, act_dim=A, hidden=H, n_hidden=NL, activation=1, row_offset=0), **kw))
    for s in ("layout", "params", "w"):
        assert act_refused(struct_null=(s,)), s
    for kw in (dict(num_rows=-1), dict(obs_dim=0), dict(goal_dim=-1), dict(obs_dim=97), dict(obs_dim=90, goal_dim=4), dict(act_dim=0), dict(act_dim=17),
               dict(hidden=32), dict(hidden=320), dict(n_hidden=1), dict(n_hidden=4), dict(activation=2), dict(row_offset=-1)):
        assert act_refused(layout=alay(**kw)), kw
    for i in list(range(8)) + [NT - 1]:
        assert act_refused(wnull=i), i
    for i in range(8, 16):
        assert act_refused(wnull=i) and act(wnull=i, value=False, work_ptr="null")[0] == -1 and b"workspace" in L.xarm_last_error(None)   # vf is read with out_value only
    for i in list(range(1, 7)) + list(range(9, 15)):
        assert act_refused(misalign=i), i
    assert act_refused(null=("calls",)) and act_refused(null=("obs",)) and act_refused(layout=alay(obs_dim=D - 6, goal_dim=3), null=("ag",))
    assert act_refused(work_ptr="null") and act_refused(work_ptr="odd")
    assert act(layout=alay(num_rows=0), null=("obs", "calls"), work_ptr="null") == (0, 0)
    assert L.xarm_acw_workspace_bytes(C.byref(alay(hidden=100)), C.byref(n)) == -1 and L.xarm_acw_workspace_bytes(C.byref(alay()), None) == -1
    assert L.xarm_acw_workspace_bytes(C.byref(alay()), C.byref(n)) == 0 and n.value == W.lib().pwh_act_workspace_bytes(C.byref(alay())) and n.value % 16 == 0


def test_act_rows_of_the_host_build_against_float64_and_across_batches():
    """the host build of the act call: a row's outputs do not depend on its batch or on how the row arrives (three parts or one), the
    deterministic action is the float64 mean to float32 chains' rounding, logp is the Gaussian's at the drawn z"""
    shape = W.SHAPE_ODD
    D, A = shape[:2]
    model = W.model_of(shape)
    w = W.weights_of(model)
    rows = np.random.RandomState(0).uniform(-2.5, 2.5, (65, D)).astype(np.float32)
    full = W.host_act(w, rows, shape, seed=3, row_offset=10)
    part = W.host_act(w, rows[40:], shape, seed=3, row_offset=50)
    split3 = W.host_act(w, rows, shape, goal_dim=3, seed=3, row_offset=10)
    for k in ("action", "env_action", "logp", "value"):
        assert PH.bits(full[k][40:]) == PH.bits(part[k]) and PH.bits(full[k]) == PH.bits(split3[k]), k
    det = W.host_act(w, rows, shape, deterministic=True)
    m64 = W.model_of(shape).double()
    with torch.no_grad():
        mean64, v64 = m64.pi(torch.from_numpy(rows).double()).numpy(), m64.value(torch.from_numpy(rows).double()).numpy()
    assert np.abs(det["action"] - mean64).max() <= 1e-4 * max(1.0, np.abs(mean64).max()) and np.abs(det["value"] - v64).max() <= 1e-4 * max(1.0, np.abs(v64).max())
    z = (full["action"].astype(np.float64) - mean64) / np.exp(model.log_std.detach().numpy().astype(np.float64))
    lp64 = (-0.5 * z * z - model.log_std.detach().numpy().astype(np.float64) - 0.5 * np.log(2 * np.pi)).sum(-1)
    assert np.abs(full["logp"] - lp64).max() <= 1e-3 and 0.5 < z.std() < 2.0


# ----------------------------------------------------------------------------------------------------------------------- driver
@pytest.mark.parametrize("algo", ("a2c", "ppo"))
def test_train_builds_the_requested_shape_on_the_scripted_env(algo, tmp_path):
    from test_train_driver import ScriptedEnv
    from gym_xarm_amd import train as TR
    model, venv, hist = TR.train(env_id="Scripted-v0", env=ScriptedEnv(16), updates=2, algo=algo, n_steps=8, quiet=True, log_every=2,
                                 net_arch=(128, 128, 128), activation="relu")
    assert model.net_arch == (128, 128, 128) and model.activation == "relu" and len(hist) == 1 and all(np.isfinite(x) for x in hist[0].values())
    path = str(tmp_path / "m.safetensors")
    TR.save_model(path, model, venv)
    back, vn = TR.load_checkpoint(path)
    assert back.net_arch == (128, 128, 128) and all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), model.state_dict().values())) and len(vn) > 0
    with pytest.raises(ValueError, match="64-64|no host path|HIP"):
        TR.train(env_id="Scripted-v0", env=ScriptedEnv(16), updates=1, algo="a2c", net_arch=(128, 128), device_update=True, quiet=True)


def test_cli_documents_the_shape_flags_for_every_algo():
    import io
    from contextlib import redirect_stdout
    from gym_xarm_amd import train as TR
    buf = io.StringIO()
    with pytest.raises(SystemExit), redirect_stdout(buf):
        TR.main(["--help"])
    text = " ".join(buf.getvalue().split())
    assert "--net-arch" in text and "sac: hidden widths" not in text and "sac: tanh" not in text


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
    """one update and one act call at (29, 1, 192, 3, tanh), 5 x 13 rows, through the host cores as a stand-alone program (its own main, never
    loaded into python)"""
    exe = str(tmp_path / "ppow_main_san")
    src = os.path.join(W.DIR, "ppow_main.cpp")
    subprocess.check_call(["g++", "-g"] + PH.gxx_flags() + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                            "-fno-omit-frame-pointer", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ppow_main ok" in r.stdout and "ERROR" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
