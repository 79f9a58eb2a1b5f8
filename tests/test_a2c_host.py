"""The A2C update core (csrc/xarm_a2c_core.h) on the CPU: the g++ build of the header against torch's float64 autograd, clip_grad_norm_
and RMSprop - returns, the gradient rule, the all-masked batch, one and three updates, the clip, the optimiser-state round trip, the
argument checks of the real library, and an address / undefined-behaviour sanitizer run of the host core as a stand-alone program.

The gradient rule (a2c_host.rule): with Y what torch's own float32 autograd loses against float64 on the same case, relative to each
tensor's largest entry and taken over the 13 tensors, every tensor obeys max|g - g64| <= 4 Y max|g64_tensor| + 2^-23 max|g64_model|.
Largest error in units of Y over these cases, host core: gradient 2.83, parameters after one update 1.75, after three 1.80 (the
tests print every case's figure; DESIGN.md 21 lists them.  Y is a property of torch's CPU kernels and varies between machines)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import a2c_host as AH
import policy_host as PH

SCALES = (1.0, 4.0)
ENT = (0.0, 0.01)


# ---------------------------------------------------------------------------------------------------------------------- returns
@pytest.mark.parametrize("T", (1, 5))
@pytest.mark.parametrize("masked", (False, True))
def test_returns_follow_the_loop_of_train_py(T, masked):
    D, A, E = 14, 4, 9
    b = AH.make_batch(D, A, T, E, 1.0, masked)
    b["done"][:] = 0.0
    b["done"][0, 0] = 1.0                      # cut at the first step
    b["done"][T // 2, 1] = 1.0                 # at a middle step
    b["done"][T - 1, 2] = 1.0                  # at the last step: the bootstrap value is cut off
    b["done"][:, 3] = 1.0                      # at every step
    w = PH.weights_of(AH.model_of(D, A, 1.0))
    boot = PH.host_act(w, b["last_obs"], D, 0, deterministic=True)["value"].astype(np.float64)   # the policy's value chain
    rc, out = AH.host_update(w, AH.zeros_like_weights(w), b, AH.hyper())
    assert rc == 0
    ret, ref, top = boot, np.zeros((T, E)), np.abs(boot)
    for k in reversed(range(T)):               # train.py:308-310 in float64
        ret = b["reward"][k].astype(np.float64) + 0.99 * ret * (1.0 - b["done"][k])
        ref[k] = ret
        top = np.maximum(top, np.abs(ret))
    # one rounding of gamma to float32 and one fused multiply-add per step
    assert np.all(np.abs(out["returns"] - ref) <= 2.0 * T * PH.ulp32(top)[None, :])
    cut = b["done"] != 0
    assert cut.sum() >= 3 and PH.bits(out["returns"][cut]) == PH.bits(b["reward"][cut])
    assert np.isfinite(out["returns"]).all() and np.isfinite(out["grad"]).all()


# --------------------------------------------------------------------------------------------------------------------- gradient
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("D,A", AH.WIDTHS)
def test_gradient_against_float64_autograd(D, A, scale):
    worst = 0.0
    for T, E in AH.SHAPES:
        for ent in ENT:
            r = AH.reference(D, A, T, E, scale, ent)
            w = PH.weights_of(AH.model_of(D, A, scale))
            rc, out = AH.host_update(w, AH.zeros_like_weights(w), r["b"], r["h"])
            assert rc == 0
            ratio, in_y = AH.rule(out["grad"], r["g64"], r["Y"], D, A)
            print("host gradient D %d A %d scale %g rows %dx%d ent %g: Y %.2e, error %.2f Y (%s, %.1e of the model's largest entry), error / bound %.3f"
                  % ((D, A, scale, T, E, ent, r["Y"], in_y) + AH.worst_tensor(out["grad"], r["g64"], D, A) + (ratio,)))
            worst = max(worst, in_y)
            assert ratio <= 1.0, (T, E, ent, ratio, in_y)
            st = out["stats"].astype(np.float64)
            ref = r["st64"]
            # a row's loss terms pass through fewer than 8 + 4 A float32 roundings on top of what the forward loses (Y's source too);
            # the sums run in float64.  n_use is a sum of zeros and ones; the entropy is A float32 values added in float64.
            rel = 4.0 * r["Y"] + (8 + 4 * A) * 2.0 ** -24
            tol = {"policy_loss": rel * ref["policy_abs"], "value_loss": rel * ref["value_loss"], "entropy": 2.0 ** -23 * max(1.0, abs(ref["entropy"])),
                   "grad_norm": rel * ref["grad_norm"], "n_use": 0.0}
            for i, k in enumerate(("policy_loss", "value_loss", "entropy", "grad_norm", "n_use")):
                assert abs(st[i] - ref[k]) <= tol[k] + 2.0 ** -24 * abs(ref[k]), (k, st[i], ref[k], tol[k])
            assert np.all(st[5:] == 0.0)
    print("host gradient D %d A %d scale %g: largest error %.2f Y" % (D, A, scale, worst))


def test_all_masked_batch_changes_nothing_but_square_avg():
    D, A, T, E = 30, 4, 5, 13
    b = AH.make_batch(D, A, T, E, 1.0)
    b["use"][:] = 0.0
    w = PH.weights_of(AH.model_of(D, A, 1.0))
    before = AH.clone_weights(w)
    sq = AH.zeros_like_weights(w)
    rs = np.random.RandomState(3)
    for k in PH.NAMES:
        sq[k][...] = rs.uniform(0.0, 0.01, sq[k].shape)
    sq0 = AH.clone_weights(sq)
    rc, out = AH.host_update(w, sq, b, AH.hyper())
    assert rc == 0 and np.all(out["grad"] == 0.0) and out["stats"][3] == 0.0 and out["stats"][4] == 1.0
    for k in PH.NAMES:
        assert PH.bits(w[k]) == PH.bits(before[k]), k
        assert PH.bits(sq[k]) == PH.bits(np.float32(0.99) * sq0[k]), k


# ------------------------------------------------------------------------------------------------------------------- parameters
def parameter_case(D, A, scale, n_updates, reward_scale, max_grad_norm=0.5):
    """float64 and float32 torch updates, the host build's updates, and the entries left out: those whose float64 gradient lies
    within the gradient bound of zero in any of the updates"""
    h = AH.hyper(max_grad_norm=max_grad_norm)
    batches = [AH.make_batch(D, A, 5, 13, scale, seed=s, reward_scale=reward_scale) for s in range(n_updates)]
    model = PH.case(D, 0, A, scale)["model"]
    w = PH.weights_of(model)
    sq = AH.zeros_like_weights(w)
    left_out = np.zeros(sum(AH.sizes(D, A)), bool)
    norms = []
    for i, b in enumerate(batches):
        m64_before, _ = AH.torch_updates(model, batches[:i], h, torch.float64)
        g64, _, st = AH.torch_grad(m64_before, b, h, torch.float64)
        g32, _, _ = AH.torch_grad(m64_before, b, h, torch.float32)
        Yg = AH.yardstick(g32, g64, D, A)
        left_out |= AH.sensitive(g64, Yg, D, A)
        rc, out = AH.host_update(w, sq, b, h)
        assert rc == 0
        norms.append((float(out["stats"][3]), st["grad_norm"], Yg))
    m64, _ = AH.torch_updates(model, batches, h, torch.float64)
    m32, _ = AH.torch_updates(model, batches, h, torch.float32)
    p32 = AH.flat_of(PH.weights_of(m32))
    p64 = np.concatenate([p.detach().numpy().ravel() for p in PH.model_params(m64)])
    return dict(p64=p64, p32=p32, p=AH.flat_of(w), left_out=left_out, norms=norms, p0=AH.flat_of(PH.weights_of(model)))


def check_parameters(c, D, A):
    for part in AH.split(c["left_out"], D, A):
        assert part.sum() <= 0.01 * part.size, "more than 1 % of a tensor's entries have a float64 gradient at zero"
    keep = ~c["left_out"]
    Y = AH.yardstick(np.where(keep, c["p32"], c["p64"]), c["p64"], D, A)
    ratio, in_y = AH.rule(c["p"], c["p64"], Y, D, A, keep)
    assert np.abs(c["p"] - c["p0"]).max() > 1e-4                    # the update moved the parameters
    return ratio, in_y, Y


@pytest.mark.parametrize("n_updates", (1, 3))
@pytest.mark.parametrize("D,A", ((14, 4), (30, 4)))
def test_updates_against_torch_clip_and_rmsprop(D, A, n_updates):
    c = parameter_case(D, A, 1.0, n_updates, 1.0)
    ratio, in_y, Y = check_parameters(c, D, A)
    print("host parameters D %d A %d after %d updates: Y %.2e, error %.2f Y, error / bound %.3f, left out %d" % (D, A, n_updates, Y, in_y, ratio, c["left_out"].sum()))
    assert ratio <= 1.0


@pytest.mark.parametrize("reward_scale,max_grad_norm,active", ((1.0, 0.5, True), (0.01, 8.0, False)))
def test_clip_active_and_inactive(reward_scale, max_grad_norm, active):
    """standard normal rewards: the norm is 26, far above 0.5; rewards of 0.01 leave 4.7 (the values the returns are compared with do
    not shrink with the rewards), under a max_grad_norm of 8"""
    D, A = 14, 4
    c = parameter_case(D, A, 1.0, 1, reward_scale, max_grad_norm)
    norm, norm64, Yg = c["norms"][0]
    assert (norm64 > max_grad_norm) == active, norm64
    assert abs(norm - norm64) <= (4.0 * Yg + 2.0 ** -22) * norm64          # the gradient's own bound, and the norm's float32 rounding
    ratio, in_y, Y = check_parameters(c, D, A)
    print("host parameters, clip %s: norm %.4f, Y %.2e, error %.2f Y" % ("active" if active else "inactive", norm64, Y, in_y))
    assert ratio <= 1.0


def test_optimizer_state_round_trip():
    """an RMSprop that has taken two steps hands its state over, the host build takes the third step, and a fresh RMSprop continues
    from the exported state with the fourth: as torch alone"""
    from gym_xarm_amd.device_a2c import export_square_avg, load_square_avg, module_params
    D, A = 14, 4
    h = AH.hyper()
    batches = [AH.make_batch(D, A, 5, 13, 1.0, seed=s) for s in range(4)]
    model = PH.case(D, 0, A, 1.0)["model"]
    m2, opt2 = AH.torch_updates(model, batches[:2], h, torch.float32)
    m3, opt3 = AH.torch_updates(model, batches[:3], h, torch.float32)
    m4, _ = AH.torch_updates(model, batches, h, torch.float32)
    sq_t = [torch.zeros_like(p) for p in module_params(m2)]
    load_square_avg(sq_t, opt2, module_params(m2))
    for s, p in zip(sq_t, module_params(m2)):
        assert torch.equal(s, opt2.state[p]["square_avg"]) and s.data_ptr() != opt2.state[p]["square_avg"].data_ptr()
    w = PH.weights_of(m2)
    sq = {k: PH.aligned(s.numpy()) for k, s in zip(PH.NAMES, sq_t)}
    rc, _ = AH.host_update(w, sq, batches[2], h)
    assert rc == 0
    # the third step's state against torch's own float32 one.  Both gradients lie within (4 + 1) Y_g of float64's relative to the
    # tensor's largest entry, a square doubles a relative error, and the clip's norm adds as much again: 16 Y_g, plus the roundings of
    # the state's own update
    g64, _, _ = AH.torch_grad(m2, batches[2], h, torch.float64)
    g32, _, _ = AH.torch_grad(m2, batches[2], h, torch.float32)
    Yg = AH.yardstick(g32, g64, D, A)
    for k, p in zip(PH.NAMES, module_params(m3)):
        ref = opt3.state[p]["square_avg"].numpy().astype(np.float64)
        assert np.abs(sq[k] - ref).max() <= (16.0 * Yg + 2.0 ** -22) * np.abs(ref).max(), k
    # export into a fresh optimiser on a module that holds the host build's parameters, and take the fourth step with torch
    m = AH.model_of(D, A, 1.0)
    with torch.no_grad():
        for k, p in zip(PH.NAMES, module_params(m)):
            p.copy_(torch.from_numpy(w[k]))
    opt = torch.optim.RMSprop(m.parameters(), lr=h["lr"], alpha=h["alpha"], eps=h["eps"])
    export_square_avg([torch.from_numpy(sq[k]) for k in PH.NAMES], opt, module_params(m))
    for k, p in zip(PH.NAMES, module_params(m)):
        assert PH.bits(opt.state[p]["square_avg"].numpy()) == PH.bits(sq[k])
    back = [torch.zeros_like(p) for p in module_params(m)]
    load_square_avg(back, opt, module_params(m))
    for k, s in zip(PH.NAMES, back):
        assert PH.bits(s.numpy()) == PH.bits(sq[k])                 # both directions, bit for bit
    loss, _, _ = AH.torch_loss(m, batches[3], h)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(m.parameters(), h["max_grad_norm"])
    opt.step()
    # the fourth step moves every entry by about lr 10 = 7e-3: continuing from the handed-over state lands on torch's own fourth step
    for p, q in zip(module_params(m), module_params(m4)):
        assert (p - q).abs().max() <= 0.02 * h["lr"] * 10
    with pytest.raises(ValueError, match="momentum"):
        load_square_avg(back, torch.optim.RMSprop(m.parameters(), momentum=0.9), module_params(m))


def test_device_class_refuses_a_cpu_model():
    from gym_xarm_amd.device_a2c import DeviceA2C
    with pytest.raises(ValueError, match="torch update of train.py"):
        DeviceA2C(AH.model_of(14, 4, 1.0), num_envs=8)


# ------------------------------------------------------------------------------------------------------------- argument checks
def test_invalid_arguments_are_refused_by_the_library():
    """every XARM_E_INVALID case of xarm_a2c_update through libxarm_hip.so itself (the checks come before any launch, so they run
    without a GPU) and through the host build, which shares the checks"""
    from gym_xarm_amd import _native
    L = _native.load()
    D, A, T, E = 14, 4, 5, 13
    b = AH.make_batch(D, A, T, E, 1.0)
    w = PH.weights_of(AH.model_of(D, A, 1.0))
    sq = AH.zeros_like_weights(w)
    work = PH.aligned(np.zeros(8, np.float32))
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(layout=None, params=None, ws=w, qs=sq, null=(), misalign=None, ws_null=False, qs_null=False, layout_null=False, params_null=False,
             work_ptr="ok"):
        layout = layout or _native.XarmA2CLayout(E, T, D, A, 64)
        params = params or AH.abi_params(AH.hyper())
        wp = {k: ws[k].ctypes.data for k in PH.NAMES}
        qp = {k: qs[k].ctypes.data for k in PH.NAMES}
        for k in null:
            if k.startswith("sq."):
                qp[k[3:]] = None
            elif k in wp:
                wp[k] = None
        if misalign:
            wp[misalign] += 4
        W, Q = _native.XarmPolicyWeights(*[wp[k] for k in PH.NAMES]), _native.XarmPolicyWeights(*[qp[k] for k in PH.NAMES])
        data = {k: (None if k in null else P(b[k])) for k in ("obs", "action", "reward", "done", "use", "last_obs")}
        wk = {"ok": P(work), "null": None, "odd": C.c_void_p(work.ctypes.data + 4)}[work_ptr]
        args = [None if layout_null else C.byref(layout), None if params_null else C.byref(params), None if ws_null else C.byref(W),
                None if qs_null else C.byref(Q), data["obs"], data["action"], data["reward"], data["done"], data["use"], data["last_obs"], wk,
                None, None, None]
        return L.xarm_a2c_update(*args, None), AH.lib().ah_update(*args)

    def refused(**kw):
        rc, rh = call(**kw)
        return rc == -1 and rh == -1 and b"xarm_a2c_update" in L.xarm_last_error(None)

    lay = lambda **kw: _native.XarmA2CLayout(**dict(dict(num_envs=E, n_steps=T, obs_dim=D, act_dim=A, hidden=64), **kw))
    par = lambda **kw: AH.abi_params(AH.hyper(**kw))
    assert refused(layout_null=True) and refused(params_null=True) and refused(ws_null=True) and refused(qs_null=True)
    for kw in (dict(num_envs=-1), dict(n_steps=0), dict(n_steps=-3), dict(obs_dim=0), dict(obs_dim=97), dict(act_dim=0), dict(act_dim=17), dict(hidden=32),
               dict(num_envs=1 << 29, n_steps=4), dict(num_envs=(1 << 31) - 1, n_steps=2)):
        assert refused(layout=lay(**kw)), kw
    for kw in (dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(lr=-1e-3), dict(alpha=-0.1), dict(alpha=1.0), dict(eps=0.0), dict(eps=-1e-5),
               dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(vf_coef=float("inf"))):
        assert refused(params=par(**kw)), kw
    for k in PH.NAMES:
        assert refused(null=(k,)), k
        assert refused(null=("sq." + k,)), k
    for k in ("pi_b1", "pi_w2", "pi_b2", "pi_w3", "vf_b1", "vf_w2", "vf_b2", "vf_w3"):
        assert refused(misalign=k), k
    for k in ("obs", "action", "reward", "done", "last_obs"):
        assert refused(null=(k,)), k
    assert refused(work_ptr="null") and refused(work_ptr="odd")
    # num_envs == 0 is a no-op that returns OK whatever the pointers are; use may be NULL (the host build runs it)
    assert call(layout=lay(num_envs=0), null=("obs", "action", "reward", "done", "last_obs"), work_ptr="null") == (0, 0)
    assert AH.host_update(w, sq, dict(b, use=None), AH.hyper())[0] == 0
    # the workspace size: refused for an unusable layout, positive and 16-byte granular otherwise, and what the host build states
    n = C.c_int64(-5)
    assert L.xarm_a2c_workspace_bytes(C.byref(lay(obs_dim=0)), C.byref(n)) == -1 and L.xarm_a2c_workspace_bytes(C.byref(lay()), None) == -1
    assert L.xarm_a2c_workspace_bytes(None, C.byref(n)) == -1
    assert L.xarm_a2c_workspace_bytes(C.byref(lay()), C.byref(n)) == 0 and n.value > 0 and n.value % 16 == 0
    assert n.value == AH.lib().ah_workspace_bytes(C.byref(lay()))


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
    """updates over the row counts and widths of these tests through the host core as a stand-alone program (its own main, never
    loaded into python)"""
    exe = str(tmp_path / "a2c_main_san")
    src = os.path.join(AH.DIR, "a2c_main.cpp")
    subprocess.check_call(["g++", "-g"] + PH.gxx_flags() + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                            "-fno-omit-frame-pointer", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "a2c_main ok" in r.stdout and "ERROR" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
