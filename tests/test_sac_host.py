"""The SAC update core (csrc/xarm_sac_core.h) on the CPU: the g++ build of the header against a torch float64 restatement of one SAC
step (tests/sac_host.py) - the actor row, the soft target, the three gradients and dq/da under the rule of tests/sac_host.py, a fixed
entropy coefficient, the clamp of log_std, the all-masked batch, the Polyak step, whole steps against three torch Adams, the
optimiser-state round trip, the argument checks of the real library, the torch SAC block of train_sac(), and an address /
undefined-behaviour sanitizer run of the host core as a stand-alone program.

The gradient rule: per tensor max|g - g64| <= 4 Y max|g64_tensor| + 2^-23 max|g64_group|, Y what torch's float32 autograd loses against
float64 on the same case.  Largest error in units of Y over these cases, host core: gradients 1.73 at weights x 1 (critic, D 88 A 8, one
row) and 1.00 at weights x 4, where the saturated tanh makes 1 - a^2 the same float32 quantity in torch and here; parameters after three
steps 1.03 (the tests print every case's figure; DESIGN.md 23 lists them.  Y is a property of torch's CPU kernels and varies between
machines)."""
import copy
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import policy_host as PH
import sac_host as SH


# --------------------------------------------------------------------------------------------------------------------- the actor row
@pytest.mark.parametrize("D,A", SH.WIDTHS)
def test_actor_row_against_float64(D, A):
    """a, logp and the deterministic action of the host build's act call against float64 from the same z: the call's Philox words,
    generated again in NumPy (tests/policy_host.py) and put through Box-Muller in float64"""
    model, h = SH.make_model(D, A), SH.hyper(seed=9)
    w = SH.weights_of(model)
    rows = SH.make_batch(D, A, 200, 1.0)["obs"]
    calls = np.array([4], np.int64)
    out = SH.host_act(w, rows, A, h, calls=calls, row_offset=17)
    assert calls[0] == 5
    # the same Philox words in NumPy (policy_host.noise_words: seed, global row, calls, column block) through float64 Box-Muller
    z64 = PH.box_muller(PH.noise_words(9, np.arange(17, 217), 4, A), np.float64)[:, :A]
    m64 = copy.deepcopy(model).double()
    with torch.no_grad():
        a64, lp64, raw = SH.actor_row(m64, torch.from_numpy(rows).double(), torch.from_numpy(z64))
        d64, _, _ = SH.actor_row(m64, torch.from_numpy(rows).double(), None, deterministic=True)
    a64, lp64, d64 = a64.numpy(), lp64.numpy(), d64.numpy()
    # u carries the forward's and the draw's float32 roundings (|u| up to ~6: 2^-21), tanh contracts; logp adds log(1 - a^2 + 1e-6), whose
    # argument 1 - a^2 carries 2^-23 absolute: relative 2^-23 / (1 - a^2 + 1e-6)
    assert np.abs(out["action"] - a64).max() <= 2.0 ** -19
    s = 1.0 - a64 ** 2 + 1e-6
    tol = 2.0 ** -17 + (2.0 ** -21 / s).sum(1)
    assert np.all(np.abs(out["logp"] - lp64) <= tol), np.abs(out["logp"] - lp64).max()
    det = SH.host_act(w, rows, A, h, deterministic=True, calls=calls)
    assert calls[0] == 5 and np.abs(det["action"] - d64).max() <= 2.0 ** -20
    assert np.all(np.abs(out["action"]) <= 1.0) and not np.array_equal(out["action"], det["action"])
    # a row does not depend on its batch, and the draw follows the global row
    part = SH.host_act(w, rows[40:100], A, h, calls=np.array([4], np.int64), row_offset=57)
    assert PH.bits(part["action"]) == PH.bits(out["action"][40:100]) and PH.bits(part["logp"]) == PH.bits(out["logp"][40:100])


# ------------------------------------------------------------------------------------------------------------------------ the target
@pytest.mark.parametrize("masked", (False, True))
def test_target_for_done_rows_and_masks(masked):
    D, A, B = 14, 4, 65
    r = SH.reference(D, A, B, 1.0, masked=masked)
    b = dict(r["b"])
    assert set(np.unique(b["done"])) == {0.0, 1.0}
    w, m, v, step = SH.fresh_state(r["model"])
    rc, out = SH.host_update(w, m, v, step, b, r["h"])
    assert rc == 0 and int(step[0]) == 1
    ratio, in_y, Y = SH.block_rule(out["y"], r["r32"]["y"], r["r64"]["y"])
    assert ratio <= 1.0
    done = b["done"] != 0
    assert PH.bits(out["y"][done]) == PH.bits(b["reward"][done])          # a done row's target is its reward: gamma (1 - done) = 0
    assert np.abs(out["y"][~done] - b["reward"][~done]).min() > 1e-3
    # y does not depend on the mask
    b2 = dict(b, use=None if masked else np.ones(B, np.float32))
    w, m, v, step = SH.fresh_state(r["model"])
    assert PH.bits(SH.host_update(w, m, v, step, b2, r["h"])[1]["y"]) == PH.bits(out["y"])


# --------------------------------------------------------------------------------------------------------------------- gradients
def host_case(r, D, A, what):
    w, m, v, step = SH.fresh_state(r["model"])
    rc, out = SH.host_update(w, m, v, step, r["b"], r["h"])
    assert rc == 0 and int(step[0]) == 1
    res = SH.rule(out["grad"], r["r64"]["grad"], r["Y"], D, A)
    by, bq = SH.block_rule(out["y"], r["r32"]["y"], r["r64"]["y"]), SH.block_rule(out["dqda"], r["r32"]["dqda"], r["r64"]["dqda"])
    print("host SAC %s: Y %.2e, error in Y: actor %.2f critic %.2f log_alpha %.2f, y %.2f, dq/da %.2f"
          % (what, r["Y"], res["actor"][1], res["critic"][1], res["log_alpha"][1], by[1], bq[1]))
    for k, (ratio, _) in res.items():
        assert ratio <= 1.0, (what, k, ratio)
    assert by[0] <= 1.0 and bq[0] <= 1.0, (what, by, bq)
    ref = r["r64"]["stats"]
    rel = 4.0 * r["Y"] + (16 + 8 * A) * 2.0 ** -24        # a row's terms pass through fewer than 16 + 8 A float32 roundings; the sums run in float64
    # a critic's output is a sum of 65 terms whose sizes add up to at most |W3|_1 + |b3|: that, not |q| (the terms cancel), is what a
    # relative rounding of the forward scales with; y carries it from the targets, with alpha logp' and the reward on top
    m = r["model"]
    l1 = max(float((t[4].weight.abs().sum() + t[4].bias.abs().sum()).detach()) for t in (m.q1, m.q2, m.q1_target, m.q2_target))
    dq = rel * (2.0 * l1 + ref["logp_abs"] + 1.0)
    tol = {"critic_loss": rel * ref["critic_loss"] + 2.0 * np.sqrt(2.0 * ref["critic_loss"]) * dq, "actor_loss": rel * ref["actor_abs"] + dq,
           "alpha_loss": rel * abs(ref["alpha_loss"]) + rel * ref["logp_abs"], "alpha": 2.0 ** -22 * ref["alpha"], "logp_pi": rel * ref["logp_abs"],
           "min_q": rel * ref["q_abs"] + dq, "n_use": 0.0}
    for i, k in enumerate(SH.STATS):
        assert abs(float(out["stats"][i]) - ref[k]) <= tol[k] + 2.0 ** -24 * abs(ref[k]), (what, k, out["stats"][i], ref[k], tol[k])
    assert out["stats"][7] == 0.0
    return max(x[1] for x in res.values()), out


@pytest.mark.parametrize("scale", (1.0, 4.0))
@pytest.mark.parametrize("D,A", SH.WIDTHS)
def test_gradients_and_action_gradient_against_float64(D, A, scale):
    worst = 0.0
    for B in SH.ROWS:
        worst = max(worst, host_case(SH.reference(D, A, B, scale), D, A, "D %d A %d B %d weights x %g" % (D, A, B, scale))[0])
    print("host SAC gradient D %d A %d weights x %g: largest error %.2f Y" % (D, A, scale, worst))


def test_fixed_entropy_coefficient_against_auto():
    D, A, B = 14, 4, 65
    _, fixed = host_case(SH.reference(D, A, B, 1.0, ent_coef=0.2), D, A, "fixed ent_coef 0.2")
    _, auto = host_case(SH.reference(D, A, B, 1.0), D, A, "auto")
    assert fixed["stats"][3] == np.float32(0.2) and fixed["stats"][2] == 0.0 and fixed["grad"][-1] == 0.0
    assert abs(auto["stats"][3] - np.exp(-0.7)) <= 2.0 ** -22 and auto["stats"][2] != 0.0 and auto["grad"][-1] != 0.0
    # a fixed coefficient leaves log_alpha and its Adam state alone
    r = SH.reference(D, A, B, 1.0, ent_coef=0.2)
    w, m, v, step = SH.fresh_state(r["model"])
    SH.host_update(w, m, v, step, r["b"], r["h"])
    assert w["log_alpha"][0] == np.float32(-0.7) and m["log_alpha"][0] == 0.0 and v["log_alpha"][0] == 0.0


def test_rows_beyond_the_upper_clamp_give_no_log_std_delta():
    """the last actor layer's bias shifted so that the rows n % 3 == 0 sit beyond log_std = 2 by at least 0.1 in every column; with those
    rows as the batch's used rows the log_std half of the last layer gets exactly zero gradient, the mean half does not"""
    D, A, B = 14, 4, 65
    r = SH.reference(D, A, B, 1.0, shift=True)
    used = r["b"]["use"] != 0
    # the third's 22 rows, less a row that sac_host.settle took out for its near-tied critics
    assert 20 <= used.sum() <= 22 and not used[np.arange(B) % 3 != 0].any() and np.all(r["r64"]["raw_log_std"][used] >= 2.1)
    _, out = host_case(r, D, A, "log_std clamped on every used row")
    g = SH.split(out["grad"], D, A)
    assert np.all(g[4].reshape(2 * A, 64)[A:] == 0.0) and np.all(g[5][A:] == 0.0)
    assert np.abs(g[4].reshape(2 * A, 64)[:A]).max() > 0.0 and np.abs(g[5][:A]).max() > 0.0
    assert np.all(SH.split(r["r64"]["grad"], D, A)[5][A:] == 0.0)          # and so says float64


def test_all_masked_batch_changes_nothing_but_the_targets_and_the_step_count():
    """every gradient is exactly zero and `step` advances.  Adam's step on a zero gradient from zero state is m = v = 0 and
    p - lr' (0 / (0 + eps)) = p: the 19 trained tensors keep their bits; the targets take their Polyak step"""
    D, A, B = 30, 4, 200
    b = SH.make_batch(D, A, B, 1.0)
    b["use"][:] = 0.0
    w, m, v, step = SH.fresh_state(SH.make_model(D, A))
    before = {k: w[k].copy() for k in SH.NAMES}
    step[0] = 7
    rc, out = SH.host_update(w, m, v, step, b, SH.hyper())
    assert rc == 0 and np.all(out["grad"] == 0.0) and int(step[0]) == 8 and out["stats"][6] == 1.0
    assert out["stats"][0] == 0.0 and out["stats"][1] == 0.0 and out["stats"][2] == 0.0
    for k in SH.TRAINED:
        assert PH.bits(w[k]) == PH.bits(before[k]) and np.all(m[k] == 0.0) and np.all(v[k] == 0.0), k
    for k, c in zip(SH.NAMES[18:30], SH.NAMES[6:18]):
        assert not np.array_equal(w[k], before[k]), k
        assert PH.bits(w[k]) == PH.bits(np.float32(0.995) * before[k] + np.float32(0.005) * before[c]), k


def test_polyak_step_against_torch_lerp():
    D, A, B = 14, 4, 65
    r = SH.reference(D, A, B, 1.0)
    w, m, v, step = SH.fresh_state(r["model"])
    before = {k: w[k].astype(np.float64) for k in SH.NAMES[18:30]}
    SH.host_update(w, m, v, step, r["b"], r["h"])
    for k, c in zip(SH.NAMES[18:30], SH.NAMES[6:18]):
        ref = torch.lerp(torch.from_numpy(before[k]), torch.from_numpy(w[c].astype(np.float64)), 0.005).numpy()     # with the stepped critic
        assert np.abs(w[k] - ref).max() <= 2.0 ** -23 * np.abs(ref).max(), k          # two products and a sum in float32


# ------------------------------------------------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("n_steps", (1, 3))
@pytest.mark.parametrize("D,A,B", ((14, 4, 65), (30, 4, 200)))
def test_whole_steps_against_three_torch_adams(D, A, B, n_steps):
    def run(model, batches, h):
        w, m, v, step = SH.fresh_state(model)
        for b in batches:
            rc, out = SH.host_update(w, m, v, step, b, h)
            assert rc == 0 and np.isfinite(out["stats"]).all()
        assert int(step[0]) == len(batches)
        return SH.flat_of(w), SH.flat_of(w, SH.NAMES[18:30])
    res, Y, left, worst_t = SH.parameter_case(D, A, B, n_steps, run)
    print("host SAC parameters D %d A %d B %d after %d steps: Y %.2e, error in Y: actor %.2f critic %.2f log_alpha %.2f, targets %.3f of the bound, left out %d"
          % (D, A, B, n_steps, Y, res["actor"][1], res["critic"][1], res["log_alpha"][1], worst_t, left))
    assert all(x[0] <= 1.0 for x in res.values()) and worst_t <= 1.0


def test_philox_noise_is_keyed_by_row_step_and_stream():
    """a NULL noise pointer: the step equals the step with the draw supplied - stream 0 for z_pi, 1 for z_next, the step counter at call
    start - which is recovered here from the NumPy Philox of tests/policy_host.py with the SAC tag"""
    D, A, B = 14, 4, 65
    b = SH.make_batch(D, A, B, 1.0)
    h = SH.hyper(seed=21)
    rows = np.arange(B, dtype=np.uint64)[:, None]
    tag = np.uint64(0x53414300)

    def draw(stream, counter):
        blk = np.arange((A + 3) // 4, dtype=np.uint64)[None, :]
        words = PH.philox(21, rows, np.uint64(0), np.uint64(counter), tag + np.uint64(4 * stream) + blk)
        return PH.box_muller(words, np.float32)[:, :A]
    outs = []
    for given in (False, True):
        model = SH.make_model(D, A)
        w, m, v, step = SH.fresh_state(model)
        step[0] = 5
        bb = dict(b, z_pi=np.ascontiguousarray(draw(0, 5)), z_next=np.ascontiguousarray(draw(1, 5)))
        rc, out = SH.host_update(w, m, v, step, bb, h, noise=given)
        assert rc == 0 and int(step[0]) == 6
        outs.append(out)
    # NumPy's float32 log / sin / cos are not the core's spelled-out ones: z agrees to a few units in the last place, y and the gradients follow
    assert np.abs(outs[0]["y"] - outs[1]["y"]).max() <= 1e-4 * max(1.0, np.abs(outs[1]["y"]).max())
    assert np.abs(outs[0]["grad"] - outs[1]["grad"]).max() <= 1e-4 * np.abs(outs[1]["grad"]).max()
    w, m, v, step = SH.fresh_state(SH.make_model(D, A))
    step[0] = 6
    other = SH.host_update(w, m, v, step, b, h, noise=False)[1]
    assert np.abs(other["y"] - outs[0]["y"]).max() > 1e-3                 # another step counter, another draw


# ------------------------------------------------------------------------------------------------------------- optimiser state
def test_optimizer_state_round_trip():
    """three torch Adams that have taken two steps hand their state over, the host build takes the third step, and fresh Adams continue
    from the exported state with the fourth: as torch alone"""
    from gym_xarm_amd.device_ppo import export_adam, load_adam
    from gym_xarm_amd.device_sac import module_params, trained
    D, A, B = 14, 4, 65
    h = SH.hyper()
    model = SH.make_model(D, A)
    batches = [SH.make_batch(D, A, B, 1.0, seed=s) for s in range(4)]
    m2, opts2, _ = SH.torch_steps(model, batches[:2], h, torch.float32)
    m3, opts3, _ = SH.torch_steps(model, batches[:3], h, torch.float32)
    m4, _, _ = SH.torch_steps(model, batches, h, torch.float32)
    groups = (("actor", slice(0, 6)), ("critic", slice(6, 18)), ("alpha", slice(18, 19)))
    ps = trained(module_params(m2))
    ea, es = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    for k, sl in groups:
        st = torch.zeros(1, dtype=torch.int64)
        load_adam(ea[sl], es[sl], st, opts2[k], ps[sl])
        assert int(st[0]) == 2
    for x, y, p, (k, sl) in zip(ea, es, ps, [g for g in groups for _ in range(g[1].stop - g[1].start)]):
        assert torch.equal(x, opts2[k].state[p]["exp_avg"]) and torch.equal(y, opts2[k].state[p]["exp_avg_sq"])
    w = SH.weights_of(m2)
    mm, vv = ({k: PH.aligned(t.numpy()) for k, t in zip(SH.TRAINED, xs)} for xs in (ea, es))
    step = np.array([2], np.int64)
    rc, _ = SH.host_update(w, mm, vv, step, batches[2], h)
    assert rc == 0 and int(step[0]) == 3
    # the third step's state against torch's own float32 one (test_ppo_host.py's bound: 16 Y_g plus the roundings of the state's update)
    _, _, r64 = SH.torch_steps(m2, [batches[2]], h, torch.float64)
    _, _, r32 = SH.torch_steps(m2, [batches[2]], h, torch.float32)
    Yg = SH.yardstick(r32[0]["grad"], r64[0]["grad"], D, A)
    for (k, sl) in groups:
        for name, p in zip(SH.TRAINED[sl], trained(module_params(m3))[sl]):
            for mine, key in ((mm, "exp_avg"), (vv, "exp_avg_sq")):
                ref = opts3[k].state[p][key].numpy().astype(np.float64)
                assert np.abs(mine[name] - ref).max() <= (16.0 * Yg + 2.0 ** -22) * np.abs(ref).max(), (name, key)
    # export into fresh optimisers on a module that holds the host build's parameters, and take the fourth step with torch
    m = copy.deepcopy(model)
    with torch.no_grad():
        for name, p in zip(SH.NAMES, module_params(m)):
            p.copy_(torch.from_numpy(w[name]))
    opts = SH.make_opts(m, h)
    pm = trained(module_params(m))
    for k, sl in groups:
        export_adam([torch.from_numpy(mm[n]) for n in SH.TRAINED[sl]], [torch.from_numpy(vv[n]) for n in SH.TRAINED[sl]], torch.from_numpy(step), opts[k], pm[sl])
        for n, p in zip(SH.TRAINED[sl], pm[sl]):
            assert PH.bits(opts[k].state[p]["exp_avg"].numpy()) == PH.bits(mm[n]) and float(opts[k].state[p]["step"]) == 3.0
        ba, bs, bt = [torch.zeros_like(p) for p in pm[sl]], [torch.zeros_like(p) for p in pm[sl]], torch.zeros(1, dtype=torch.int64)
        load_adam(ba, bs, bt, opts[k], pm[sl])
        assert int(bt[0]) == 3
        for n, x, y in zip(SH.TRAINED[sl], ba, bs):
            assert PH.bits(x.numpy()) == PH.bits(mm[n]) and PH.bits(y.numpy()) == PH.bits(vv[n])          # both directions, bit for bit
    SH.torch_step(m, opts, batches[3], h)
    for p, q in zip(trained(module_params(m)), trained(module_params(m4))):
        assert (p - q).abs().max() <= 0.05 * h["lr"]


def test_device_class_refuses_a_cpu_model():
    from gym_xarm_amd.device_sac import DeviceSAC
    with pytest.raises(ValueError, match="torch block of train_sac"):
        DeviceSAC(SH.make_model(14, 4), 256)


# ------------------------------------------------------------------------------------------------------------- argument checks
def test_invalid_arguments_are_refused_by_the_library():
    """every XARM_E_INVALID case of xarm_sac_update / xarm_sac_act through libxarm_hip.so itself (the checks come before any launch, so
    they run without a GPU) and through the host build, which shares the checks"""
    from gym_xarm_amd import _native
    L = _native.load()
    D, A, B = 14, 4, 65
    b = SH.make_batch(D, A, B, 1.0)
    w, m, v, step = SH.fresh_state(SH.make_model(D, A))
    work = PH.aligned(np.zeros(8, np.float32))
    calls = np.zeros(1, np.int64)
    out_a = np.zeros((B, A), np.float32)
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def structs(null=(), misalign=None):
        S = {"w": SH.abi_weights(w), "m": SH.abi_weights(m, SH.TRAINED), "v": SH.abi_weights(v, SH.TRAINED)}
        for k in null:
            if "." in k:
                s, name = k.split(".")
                i = SH.NAMES.index(name)
                if i == 30:
                    S[s].log_alpha = None
                else:
                    getattr(S[s], SH.TOWERS[i // 6])[i % 6] = None
        if misalign:
            i = SH.NAMES.index(misalign)
            getattr(S["w"], SH.TOWERS[i // 6])[i % 6] = w[misalign].ctypes.data + 4
        return S

    def call(layout=None, params=None, null=(), misalign=None, struct_null=(), work_ptr="ok"):
        layout = layout or SH.abi_layout(B, D, A)
        params = params or SH.abi_params(SH.hyper(), A)
        S = structs(null, misalign)
        data = {k: (None if k in null else P(b[k])) for k in ("obs", "next_obs", "action", "reward", "done", "use")}
        wk = {"ok": P(work), "null": None, "odd": C.c_void_p(work.ctypes.data + 4)}[work_ptr]
        args = [None if "layout" in struct_null else C.byref(layout), None if "params" in struct_null else C.byref(params)] + \
               [None if s in struct_null else C.byref(S[s]) for s in "wmv"] + \
               [None if "step" in null else P(step), data["obs"], data["next_obs"], data["action"], data["reward"], data["done"], data["use"], None, None, wk,
                None, None, None, None]
        return L.xarm_sac_update(*args, None), SH.lib().sh_update(*args)

    def refused(**kw):
        rc, rh = call(**kw)
        return rc == -1 and rh == -1 and b"xarm_sac_update" in L.xarm_last_error(None)

    lay = lambda **kw: _native.XarmSACLayout(**dict(dict(batch_size=B, obs_dim=D, act_dim=A, hidden=64, row_offset=0), **kw))
    par = lambda **kw: SH.abi_params(SH.hyper(**kw), A)
    for s in ("layout", "params", "w", "m", "v"):
        assert refused(struct_null=(s,)), s
    for kw in (dict(batch_size=-1), dict(obs_dim=0), dict(obs_dim=97), dict(act_dim=0), dict(act_dim=9), dict(obs_dim=88, act_dim=9), dict(obs_dim=89, act_dim=8),
               dict(obs_dim=93, act_dim=4), dict(hidden=32), dict(row_offset=-1)):
        assert refused(layout=lay(**kw)), kw
    assert call(layout=lay(obs_dim=88, act_dim=8), work_ptr="null")[0] == -1 and b"workspace" in L.xarm_last_error(None)    # D + A = 96 passes the layout check
    for kw in (dict(gamma=-0.1), dict(gamma=1.5), dict(gamma=float("nan")), dict(lr=-1e-3), dict(lr=float("inf")), dict(tau=-0.1), dict(tau=1.5),
               dict(tau=float("nan")), dict(ent_coef=-0.2), dict(ent_coef=float("inf")), dict(ent_coef=float("nan")), dict(target_entropy=float("nan")),
               dict(target_entropy=float("inf")), dict(beta1=-0.1), dict(beta1=1.0), dict(beta2=1.0), dict(beta2=float("nan")), dict(eps=0.0), dict(eps=-1e-8)):
        assert refused(params=par(**kw)), kw
    for name in SH.NAMES:
        assert refused(null=("w." + name,)), name
    for name in SH.TRAINED:
        assert refused(null=("m." + name,)) and refused(null=("v." + name,)), name
    for t in SH.TOWERS:
        for k in ("b1", "w2", "b2", "w3"):
            assert refused(misalign="%s_%s" % (t, k)), (t, k)
    for k in ("obs", "next_obs", "action", "reward", "done", "step"):
        assert refused(null=(k,)), k
    assert refused(work_ptr="null") and refused(work_ptr="odd")
    # batch_size == 0 is a no-op that returns OK whatever the pointers are
    assert call(layout=lay(batch_size=0), null=("obs", "next_obs", "action", "reward", "done", "step"), work_ptr="null") == (0, 0)

    # xarm_sac_act
    def act(layout=None, params=None, weights="ok", null=(), misalign=None):
        layout = layout or SH.abi_layout(B, D, A)
        params = params or SH.abi_params(SH.hyper(), A)
        S = structs(["w." + k for k in null if k in SH.NAMES], misalign)["w"]
        args = [C.byref(layout) if layout != "null" else None, C.byref(params) if params != "null" else None, C.byref(S) if weights == "ok" else None,
                None if "calls" in null else P(calls), None if "obs" in null else P(b["obs"]), None if "action" in null else P(out_a), None]
        return L.xarm_sac_act(*args, None), SH.lib().sh_act(*args)
    assert act(layout="null") == (-1, -1) and act(params="null") == (-1, -1) and act(weights=None) == (-1, -1)
    assert b"xarm_sac_act" in L.xarm_last_error(None)
    for kw in (dict(batch_size=-1), dict(obs_dim=0), dict(act_dim=9), dict(obs_dim=93, act_dim=4), dict(hidden=32), dict(row_offset=-1)):
        assert act(layout=lay(**kw)) == (-1, -1), kw
    for name in SH.NAMES[:6]:
        assert act(null=(name,)) == (-1, -1), name
    for k in ("actor_b1", "actor_w2", "actor_b2", "actor_w3"):
        assert act(misalign=k) == (-1, -1), k
    for k in ("calls", "obs", "action"):
        assert act(null=(k,)) == (-1, -1), k
    assert act(layout=lay(batch_size=0), null=("calls", "obs", "action")) == (0, 0)
    # the workspace size: refused for an unusable layout, positive and 16-byte granular otherwise, and what the host build states
    n = C.c_int64(-5)
    assert L.xarm_sac_workspace_bytes(C.byref(lay(act_dim=9)), C.byref(n)) == -1 and L.xarm_sac_workspace_bytes(C.byref(lay()), None) == -1
    assert L.xarm_sac_workspace_bytes(None, C.byref(n)) == -1
    assert L.xarm_sac_workspace_bytes(C.byref(lay()), C.byref(n)) == 0 and n.value > 0 and n.value % 16 == 0
    assert n.value == SH.lib().sh_workspace_bytes(C.byref(lay()))
    assert SH.geometry(16385, D, A) == [257, 256, 64, 256, 64 * D + 64 + 4096 + 64 + 128 * A + 2 * A, 64 * (D + A) + 64 + 4096 + 64 + 64 + 1, 6]
    assert SH.lib().sh_param_count(C.byref(lay())) == sum(SH.sizes(D, A))


# ----------------------------------------------------------------------------------------------------------------------- driver
def scripted_goal_env(E):
    """tests/test_train_driver.py's ScriptedEnv with what a HER buffer asks of a goal env"""
    from test_train_driver import ScriptedEnv

    class GoalEnv(ScriptedEnv):
        max_episode_steps = 6

        def __init__(self, E):
            super().__init__(E)
            self.action_dim = self.act_dim

        def compute_reward(self, achieved_goal, goal, info):
            return -((achieved_goal - goal).norm(dim=-1) > 0.75).float()
    return GoalEnv(E)


def test_train_sac_runs_the_torch_block_on_the_scripted_env():
    """40 steps of 16 envs: the buffer fills, 28 SAC steps of 32 rows run, the stats are finite and the parameters moved"""
    from gym_xarm_amd.sac import SacPolicy, train_sac
    model, venv, hist = train_sac(env_id="Scripted-v0", env=scripted_goal_env(16), steps=40, batch_size=32, quiet=True, log_every=20, seed=0)
    assert len(hist) == 2 and hist[-1]["env_steps"] == 40 * 16 and hist[-1]["updates"] == 28 and hist[0]["updates"] == 8
    for rec in hist:
        assert all(np.isfinite(x) for x in rec.values()), rec
    assert set(SH.STATS) <= set(hist[-1]) and hist[-1]["n_use"] == 32.0 and 0.0 < hist[-1]["alpha"] < 1.0
    assert venv.buffer.t == 40 and venv.buffer.num_valid() > 0 and venv.monitor.n > 16
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    torch.manual_seed(0)
    start = SacPolicy(venv.dim, 2)
    moved = max(float((p - q).detach().abs().max()) for p, q in zip(model.parameters(), start.parameters()))
    assert 1e-4 < moved <= 28 * 1e-3 * 1.5              # 28 Adam steps of about lr each
    # targets trail their critics; a fixed coefficient leaves log_alpha alone; gradient_steps and train_freq
    assert not torch.equal(model.q1_target[0].weight, model.q1[0].weight)
    model, venv, hist = train_sac(env_id="Scripted-v0", env=scripted_goal_env(16), steps=24, batch_size=32, quiet=True, log_every=24, ent_coef=0.1,
                                  gradient_steps=2, train_freq=4)
    assert float(model.log_alpha.detach()) == 0.0 and hist[-1]["alpha"] == pytest.approx(0.1) and hist[-1]["updates"] == 2 * 3
    with pytest.raises(ValueError, match="torch block of train_sac"):
        train_sac(env_id="Scripted-v0", env=scripted_goal_env(16), steps=2, quiet=True, device_update=True)


def test_cli_dispatches_sac(monkeypatch):
    """python -m gym_xarm_amd.train --algo sac reaches train_sac with --batch-size, --gradient-steps and --device-update; a2c / ppo go
    to train() as before"""
    import gym_xarm_amd.sac as sac
    import gym_xarm_amd.train as tr
    seen = {}
    monkeypatch.setattr(sac, "train_sac", lambda *a, **kw: seen.update(sac=(a, kw)) or (None, None, []))
    monkeypatch.setattr(tr, "train", lambda *a, **kw: seen.update(train=(a, kw)) or (None, None, []))
    monkeypatch.setattr("sys.argv", ["train", "--algo", "sac", "--env", "XarmReach-v0", "--num-envs", "64", "--updates", "100", "--batch-size", "128",
                                     "--gradient-steps", "2", "--device-update", "--reward-type", "sparse"])
    tr.main()
    a, kw = seen["sac"]
    assert "train" not in seen and kw["batch_size"] == 128 and kw["gradient_steps"] == 2 and kw["device_update"] is True and kw["steps"] == 100
    assert kw["num_envs"] == 64 and kw["config"]["reward_type"] == "sparse"
    monkeypatch.setattr("sys.argv", ["train", "--algo", "ppo", "--updates", "3"])
    tr.main()
    assert seen["train"][1]["algo"] == "ppo"


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
    """steps and act calls over the row counts and widths of these tests through the host core as a stand-alone program (its own main,
    never loaded into python)"""
    exe = str(tmp_path / "sac_main_san")
    src = os.path.join(SH.DIR, "sac_main.cpp")
    subprocess.check_call(["g++", "-g"] + PH.gxx_flags() + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                            "-fno-omit-frame-pointer", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sac_main ok" in r.stdout and "ERROR" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
