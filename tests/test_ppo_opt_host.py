"""The PPO options - clip_range_vf and the device-side target_kl stop (include/xarm_hip.h xarm_ppo_options) - on the CPU:
both cores' host builds (tests/hostbuild_ppo_opt) against train.py's torch block in float64, the options' invisibility when they never
act, the stop's bookkeeping, the refusals, train()'s schedules, and the sanitizer run.  Helpers, cases and their validity conditions:
tests/ppo_opt_host.py.  The GPU side is tests/test_ppo_opt_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import policy_host as PH
import ppo_host as PP
import ppo_opt_host as O
import ppow_host as W

CASES = O.TILE + O.WIDE


# ------------------------------------------------------------------------------------------------------------------- value clipping
@pytest.mark.parametrize("c", CASES, ids=O.case_id)
def test_value_clip_whole_update_against_float64(c):
    """a whole update with clip_range_vf: parameters under ppo_host.parameter_case's rule against torch float64, every stats row within
    check_stats's bounds.  The case is valid when, in float64, no used row lies within 1e-4 of the clip's edge at any step and between a
    quarter and three quarters of the used row-steps behind step 0 are clipped (asserted)"""
    c_vf = O.SETTINGS[c]["c_vf"]
    r = O.reference(c, "spread", clip_range_vf=c_vf)
    O.assert_valid_clip(r["r64"]["recs"], r["h"], c_vf)
    edge, share = O.clip_shares(r["r64"]["recs"], c_vf)
    state = O.fresh_state(c)
    before = O.flat_of(c, state[0])
    rc, out = O.host_update(c, state, r["h"], r["perm"], r["old_logp"], O.options(clip_range_vf=c_vf))
    assert rc == 0 and int(state[3][0]) == O.steps_of(c) and np.all(out["stats"][:, 7] == 0)
    p = O.flat_of(c, state[0])
    ratio, in_y, Y, left = O.parameter_rule(c, r, p)
    print("host PPO with clip_range_vf %g, %s: closest row %.1e from the edge, %.0f %% of the row-steps clipped; parameters after %d steps: Y %.2e, "
          "error %.2f Y, error / bound %.3f, left out %d" % (c_vf, O.case_id(c), edge, 100 * share, O.steps_of(c), Y, in_y, ratio, left))
    assert np.abs(p - before).max() > 1e-4 and ratio <= 1.0
    O.check_rows(c, r, out["stats"])


def test_value_clip_changes_the_update():
    """the same call without the option gives other parameters: the clip is not a no-op on these cases"""
    c = O.TILE[0]
    h, perm = PP.hyper(lr=O.LR), O.perm_of(c)
    a, b = O.fresh_state(c), O.fresh_state(c)
    assert O.host_update(c, a, h, perm, None, O.options(clip_range_vf=O.SETTINGS[c]["c_vf"]))[0] == 0 and O.host_update(c, b, h, perm)[0] == 0
    assert not O.same_bits(O.state_arrays(c, a)[:13], O.state_arrays(c, b)[:13])


# --------------------------------------------------------------------------------------------------------------- inactive options
@pytest.mark.parametrize("c", CASES, ids=O.case_id)
def test_options_that_never_act_are_invisible(c):
    """clip_range_vf = target_kl = 1e30 against options = NULL: weights, Adam state, step, adv, returns, grad and stats bit for bit"""
    h, perm = PP.hyper(lr=O.LR, ent_coef=0.01), O.perm_of(c)
    runs = []
    for opts in (None, O.options(1e30, 1e30)):
        state = O.fresh_state(c)
        rc, out = O.host_update(c, state, h, perm, None, opts)
        assert rc == 0 and int(state[3][0]) == O.steps_of(c)
        runs.append(O.state_arrays(c, state) + [out[k] for k in ("adv", "returns", "grad", "stats")])
    assert all(np.isfinite(x).all() for x in runs[0]) and O.same_bits(*runs)


def test_null_options_are_the_existing_host_builds():
    """options = NULL through the new build equals tests/hostbuild_ppo and tests/hostbuild_ppow, which compile against the same headers
    unchanged"""
    for c in (O.TILE[0], O.WIDE[0]):
        h, perm = PP.hyper(lr=O.LR), O.perm_of(c)
        mine, theirs = O.fresh_state(c), O.fresh_state(c)
        rc, out = O.host_update(c, mine, h, perm)
        if c[0] == "tile":
            rc2, out2 = PP.host_update(*theirs, O.batch_of(c), h, perm, c[5])
        else:
            rc2, out2 = W.host_update(*theirs, O.batch_of(c), h, perm, c[5], O.shape_of(c))
        assert rc == 0 and rc2 == 0
        assert O.same_bits(O.state_arrays(c, mine) + [out["stats"], out["grad"]], O.state_arrays(c, theirs) + [out2["stats"], out2["grad"]])


# ------------------------------------------------------------------------------------------------------------------------ KL stop
def stop_case(c, target_kl, old_logp):
    """the reference with target_kl (valid: assert_valid_stop), the host build's stopped call checked against it, and the bits of a call
    that ends after step s* - 1.  Returns s*"""
    r = O.reference(c, old_logp, target_kl=target_kl)
    s_star = O.assert_valid_stop(r, target_kl, c[2])
    S = O.steps_of(c)
    state = O.fresh_state(c)
    rc, out = O.host_update(c, state, r["h"], r["perm"], r["old_logp"], O.options(target_kl=target_kl))
    st = out["stats"]
    assert rc == 0 and int(state[3][0]) == s_star, (int(state[3][0]), s_star)
    assert st[:, 7].tolist() == [0.0] * s_star + [1.0] * (S - s_star), st[:, 7]
    O.check_rows(c, r, st)
    assert np.isfinite(out["grad"]).all() and (s_star > 0 or np.abs(out["grad"]).max() > 0)       # step 0's gradient is written also when step 0 trips
    # nothing past the stop touched the weights or Adam's state: a call whose layout ends after step s* - 1
    cut = O.fresh_state(c)
    assert O.host_update(c, cut, r["h"], r["perm"], r["old_logp"], None, max_steps=s_star)[0] == 0
    assert O.same_bits(O.state_arrays(c, state), O.state_arrays(c, cut))
    if s_star > 0:
        ratio, in_y, Y, left = O.parameter_rule(c, r, O.flat_of(c, state[0]))
        print("host PPO with target_kl %g, %s: trips at step %d of %d; parameters: Y %.2e, error %.2f Y, error / bound %.3f, left out %d"
              % (target_kl, O.case_id(c), s_star, S, Y, in_y, ratio, left))
        assert ratio <= 1.0
    else:
        assert O.same_bits(O.state_arrays(c, state)[:-1], O.state_arrays(c, O.fresh_state(c))[:-1])   # nothing was applied
    return s_star


@pytest.mark.parametrize("c", CASES, ids=O.case_id)
def test_kl_stop_inside_an_epoch(c):
    S, M = O.steps_of(c), O.steps_of(c) // c[6]
    s_star = stop_case(c, O.SETTINGS[c]["mid"], None)
    assert 1 <= s_star <= S - 2 and s_star % M != 0


@pytest.mark.parametrize("c", [c for c in CASES if O.SETTINGS[c]["epoch"] is not None], ids=O.case_id)
def test_kl_stop_on_the_first_step_of_an_epoch(c):
    S, M = O.steps_of(c), O.steps_of(c) // c[6]
    s_star = stop_case(c, O.SETTINGS[c]["epoch"], None)
    assert 1 <= s_star <= S - 2 and s_star % M == 0


@pytest.mark.parametrize("c", CASES, ids=O.case_id)
def test_kl_stop_at_step_zero_with_a_supplied_old_logp(c):
    """ppo_host.spread_old_logp puts two thirds of the rows outside the clip range: approx_kl of step 0 is 0.05 - 0.08"""
    assert stop_case(c, 0.02, "spread") == 0


def test_both_options_together():
    """the value clip moves the trajectory, the stop follows it: against float64 with both"""
    c = O.TILE[0]
    c_vf, kl = O.SETTINGS[c]["c_vf"], O.SETTINGS[c]["epoch"]
    r = O.reference(c, None, clip_range_vf=c_vf, target_kl=kl)
    s_star = O.assert_valid_stop(r, kl, c[2])
    state = O.fresh_state(c)
    rc, out = O.host_update(c, state, r["h"], r["perm"], None, O.options(c_vf, kl))
    assert rc == 0 and int(state[3][0]) == s_star >= 1
    O.check_rows(c, r, out["stats"])
    assert O.parameter_rule(c, r, O.flat_of(c, state[0]))[0] <= 1.0


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_bad_options_are_refused_with_a_message():
    """negative, NaN and infinite options: XARM_E_INVALID from xarm_ppo_update_opt and xarm_ppow_update_opt (the check comes before any
    launch, so it runs without a GPU) with the option's name in xarm_last_error, and -1 from the host builds"""
    from gym_xarm_amd import _native
    L = _native.load()
    assert C.sizeof(_native.XarmPPOOptions) == 16 and C.sizeof(_native.XarmPPOParams) == 88
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    for c in (O.TILE[0], O.WIDE[0]):
        kind, D, A, T, E, B, epochs = c[:7]
        b, perm = O.batch_of(c), O.perm_of(c)
        w, m, v, step = O.fresh_state(c)
        work = PH.aligned(np.zeros(1 << 16, np.float32))
        if kind == "tile":
            layout, fn, name = PP.abi_layout(T, E, D, A, epochs, B), L.xarm_ppo_update_opt, b"xarm_ppo_update"
            S3 = [_native.XarmPolicyWeights(*[x[k].ctypes.data for k in PH.NAMES]) for x in (w, m, v)]
        else:
            layout, fn, name = W.abi_layout(T, E, O.shape_of(c), epochs, B), L.xarm_ppow_update_opt, b"xarm_ppow_update"
            S3 = [W.abi_weights(x) for x in (w, m, v)]
        args = [C.byref(layout), C.byref(PP.abi_params(PP.hyper()))] + [C.byref(s) for s in S3] + \
               [P(step), P(b["obs"]), P(b["action"]), P(b["reward"]), P(b["done"]), P(b["use"]), P(b["last_obs"]), None, P(perm), P(work), None, None, None, None]
        for field, word in (("clip_range_vf", b"clip_range_vf"), ("target_kl", b"target_kl")):
            for bad in (-0.1, -1e-30, float("nan"), float("inf"), -float("inf")):
                opts = _native.XarmPPOOptions(**{field: bad})
                assert fn(*args, C.byref(opts), None) == -1, (kind, field, bad)
                msg = L.xarm_last_error(None)
                assert name in msg and word in msg, msg
                assert O.host_update(c, O.fresh_state(c), PP.hyper(), perm, None, opts)[0] == -1
        # zeros are "off" and pass the check: with num_envs == 0 the call launches nothing and returns OK
        args[0] = C.byref(PP.abi_layout(T, 0, D, A, epochs, B) if kind == "tile" else W.abi_layout(T, 0, O.shape_of(c), epochs, B))
        assert fn(*args, C.byref(_native.XarmPPOOptions(0.0, 0.0)), None) == 0 and fn(*args, None, None) == 0


def test_device_class_and_torch_learner_take_the_options():
    import inspect
    from gym_xarm_amd.device_ppo import DevicePPO
    from gym_xarm_amd import train as TR
    for f in (DevicePPO.__init__, TR.TorchPPO.__init__, TR.ppo_update, TR.train):
        sig = inspect.signature(f).parameters
        assert sig["clip_range_vf"].default is None and sig["target_kl"].default is None, f
    sig = inspect.signature(TR.ppo_minibatch_loss).parameters
    assert sig["clip_range_vf"].default is None and sig["old_values"].default is None
    with pytest.raises(ValueError, match="old_values"):
        m = PP.AH.model_of(14, 4, 1.0)
        b = PP.make_batch(14, 4, 5, 13, 1.0)
        h = PP.hyper()
        TR.ppo_minibatch_loss(m, PP.AH.rollout_of(b, torch.float32)[0], PP.torch_prepare(m, b, h), torch.arange(10), clip_range_vf=0.1)


def test_torch_block_stops_and_clips_like_the_reference_loop():
    """train.ppo_update with both options on a seeded randperm: it applies as many steps as the step-by-step loop of the tests on the
    same permutations, and ends on the same parameters"""
    from gym_xarm_amd import train as TR
    c = O.TILE[0]
    kind, D, A, T, E, B, epochs = c
    h, b = PP.hyper(lr=O.LR), O.batch_of(c)
    c_vf, kl = O.SETTINGS[c]["c_vf"], O.SETTINGS[c]["epoch"]
    torch.manual_seed(5)
    perm = np.stack([torch.randperm(T * E).numpy() for _ in range(epochs)]).astype(np.int32)
    ref = O.torch_run(c, h, perm, torch.float32, None, c_vf, kl)
    assert ref["stop"] is not None and 1 <= ref["stop"] < epochs * 4
    m = O.model_of(c)
    opt = torch.optim.Adam(m.parameters(), lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"])
    rollout, last = PP.AH.rollout_of(b, torch.float32)
    torch.manual_seed(5)
    applied = TR.ppo_update(m, opt, rollout, last, epochs, B, h["gamma"], h["gae_lambda"], h["clip_range"], h["vf_coef"], h["ent_coef"], h["max_grad_norm"],
                            True, clip_range_vf=c_vf, target_kl=kl)
    assert applied == ref["stop"]
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), ref["model"].parameters()))


# --------------------------------------------------------------------------------------------------------------------- schedules
def test_linear_schedule_values():
    from gym_xarm_amd.train import linear_schedule
    f = linear_schedule(3e-4)
    assert f(1.0) == 3e-4 and f(0.0) == 0.0 and f(0.5) == 0.5 * 3e-4 and f(0.25) == 0.25 * 3e-4


@pytest.mark.parametrize("algo", ("a2c", "ppo"))
def test_train_evaluates_schedules_at_one_minus_it_over_updates(algo, monkeypatch):
    from test_train_driver import ScriptedEnv
    from gym_xarm_amd import train as TR
    calls, seen = [], []
    cls = TR.TorchPPO if algo == "ppo" else TR.TorchA2C
    real = TR._TorchLearner.set_hyper

    def spy(self, **kw):
        calls.append(dict(kw))
        real(self, **kw)
        seen.append([g["lr"] for g in self.opt.param_groups])
    monkeypatch.setattr(cls, "set_hyper", spy)
    progress = []
    lr = lambda p: (progress.append(p), 1e-3 * p)[1]
    kw = dict(clip_range=TR.linear_schedule(0.2), clip_range_vf=lambda p: 0.05 + 0.1 * p, n_epochs=2, batch_size=48) if algo == "ppo" else {}
    updates = 4
    TR.train(env_id="Scripted-v0", env=ScriptedEnv(16), updates=updates, algo=algo, n_steps=8, lr=lr, quiet=True, log_every=updates, **kw)
    want = [1.0 - it / updates for it in range(1, updates + 1)]
    assert progress == [1.0] + want and want[-1] == 0.0                      # built with f(1), then just before each update; the last one runs at 0
    assert [c["lr"] for c in calls] == [1e-3 * p for p in want] and all(s == [1e-3 * p] for s, p in zip(seen, want))
    if algo == "ppo":
        assert [c["clip_range"] for c in calls] == [0.2 * p for p in want] and [c["clip_range_vf"] for c in calls] == [0.05 + 0.1 * p for p in want]
    else:
        assert all(sorted(c) == ["lr"] for c in calls)


@pytest.mark.parametrize("algo", ("a2c", "ppo"))
def test_float_arguments_never_pass_through_set_hyper_and_equal_a_constant_schedule(algo, monkeypatch):
    """floats take the code path they always took - set_hyper is not called - and a schedule that returns the same constants ends on the
    same parameters bit for bit"""
    from test_train_driver import ScriptedEnv
    from gym_xarm_amd import train as TR
    calls = []
    real = TR._TorchLearner.set_hyper
    monkeypatch.setattr(TR._TorchLearner, "set_hyper", lambda self, **kw: (calls.append(kw), real(self, **kw))[1])
    extra = dict(n_epochs=2, batch_size=48) if algo == "ppo" else {}
    run = lambda **kw: TR.train(env_id="Scripted-v0", env=ScriptedEnv(16), updates=3, algo=algo, n_steps=8, quiet=True, log_every=3, seed=4, **extra, **kw)[0]
    a = run(lr=5e-4, **(dict(clip_range=0.15) if algo == "ppo" else {}))
    assert calls == []
    b = run(lr=lambda p: 5e-4, **(dict(clip_range=lambda p: 0.15) if algo == "ppo" else {}))
    assert len(calls) == 3
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    c = run()                                                                      # the defaults are floats too
    assert len(calls) == 3 and any(not torch.equal(p, q) for p, q in zip(a.parameters(), c.parameters()))


def test_set_hyper_rejects_unknown_keys():
    from gym_xarm_amd import train as TR
    from gym_xarm_amd.device_a2c import DeviceA2C
    from gym_xarm_amd.device_ppo import DevicePPO
    m = TR.ActorCritic(6, 2)
    for learner in (TR.TorchA2C(m, 4), TR.TorchPPO(m, 4)):
        learner.set_hyper(lr=1e-5, gamma=0.9)
        assert learner.opt.param_groups[0]["lr"] == 1e-5 and learner.hyper["gamma"] == 0.9
        with pytest.raises(KeyError, match="learning_rate"):
            learner.set_hyper(learning_rate=1e-3)
    TR.TorchPPO(m, 4).set_hyper(clip_range=0.1, clip_range_vf=0.3, target_kl=0.01)
    with pytest.raises(KeyError, match="clip_range"):
        TR.TorchA2C(m, 4).set_hyper(clip_range=0.1)
    # the device learners' set_hyper is the same dictionary rule; the classes need a GPU to construct, the method does not
    for cls, keys in ((DevicePPO, ("lr", "clip_range", "clip_range_vf", "target_kl")), (DeviceA2C, ("lr", "gamma"))):
        obj = cls.__new__(cls)
        obj.hyper = {k: 1.0 for k in keys}
        obj.set_hyper(lr=2.0)
        assert obj.hyper["lr"] == 2.0
        with pytest.raises(KeyError, match="learning_rate"):
            obj.set_hyper(learning_rate=1e-3)


def test_train_reports_applied_steps_and_refuses_misuse():
    from test_train_driver import ScriptedEnv
    from gym_xarm_amd import train as TR
    _, _, hist = TR.train(env_id="Scripted-v0", env=ScriptedEnv(16), updates=3, algo="ppo", n_steps=8, n_epochs=2, batch_size=48, quiet=True, log_every=1,
                          target_kl=1e-7, clip_range_vf=0.2, lr=TR.linear_schedule(3e-4))
    applied = [rec["ppo_steps_applied"] for rec in hist]
    # step 0 of an update has approx_kl 0 and is applied; a step of lr 2e-4 or 1e-4 moves approx_kl past 1.5e-7; the last update runs at
    # lr 0, where nothing moves and nothing trips
    assert 1 <= applied[0] < 6 and 1 <= applied[1] < 6 and applied[2] == 6, applied
    _, _, hist = TR.train(env_id="Scripted-v0", env=ScriptedEnv(16), updates=1, algo="ppo", n_steps=8, quiet=True, log_every=1)
    assert "ppo_steps_applied" not in hist[0]
    with pytest.raises(ValueError, match="PPO"):
        TR.train(env_id="Scripted-v0", env=ScriptedEnv(16), updates=1, algo="a2c", target_kl=0.01, quiet=True)


def test_cli_documents_the_new_flags(capsys):
    from gym_xarm_amd import train as TR
    with pytest.raises(SystemExit):
        TR.main(["--help"])
    text = capsys.readouterr().out
    for flag in ("--target-kl", "--clip-range-vf", "--lr-schedule", "--clip-range-schedule"):
        assert flag in text
    with pytest.raises(SystemExit):
        TR.main(["--algo", "a2c", "--target-kl", "0.02"])


# ---------------------------------------------------------------------------------------------------------------------- sanitizers
def _have_sanitizers():
    """libasan / libubsan are installed and a sanitized program starts in this environment"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "san_probe")
        return subprocess.run(["g++", "-x", "c++", "-", "-fsanitize=address,undefined", "-o", exe], input=b"int main(){return 0;}",
                              capture_output=True).returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason="libasan/libubsan not available")
def test_options_path_of_both_cores_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the options path of both cores over the shapes of these tests as a stand-alone program (its own main, never loaded into python)"""
    exe = str(tmp_path / "ppo_opt_main_san")
    src = os.path.join(O.DIR, "ppo_opt_main.cpp")
    subprocess.check_call(["g++", "-g"] + PH.gxx_flags() + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                            "-fno-omit-frame-pointer", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ppo_opt_main ok" in r.stdout and "ERROR" not in r.stderr, (r.stdout[-2000:], r.stderr[-4000:])
