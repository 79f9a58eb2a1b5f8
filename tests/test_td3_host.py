"""CPU tests of the TD3 learner: the torch block (gym_xarm_amd/td3.py), the g++ build of csrc/xarm_td3_core.h
(tests/hostbuild_td3) against float64 torch under sacw_host's gradient rule, whole steps with the delay, the smaller cases, the argument
checks of the real library (they come before any launch), DeviceTD3's errors, the driver, the shared driver loop's golden guard, the
CLI and an address / undefined-behaviour sanitizer run of the host core as a stand-alone program.

The gradient rule: per tensor max|g - g64| <= 4 Y max|g64_tensor| + 2^-23 max|g64_group|, Y what torch's float32 autograd loses against
float64 on the same case (tests/td3_host.py)."""
import copy
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import policy_host as PH
import td3_host as TH
import sacw_host as WH

A_, REF = TH.SHAPE_A, TH.SHAPE_REF


# ----------------------------------------------------------------------------------------------------------------------- module
def test_default_module_creates_its_parameters_in_a_pinned_order():
    from gym_xarm_amd.td3 import Td3Policy
    m = Td3Policy(14, 4)
    keys = list(m.state_dict().keys())
    want = ["%s.%d.%s" % (t, i, k) for t in ("actor", "q1", "q2", "actor_target", "q1_target", "q2_target") for i in (0, 2, 4) for k in ("weight", "bias")]
    assert keys == want
    assert hashlib.sha256("\n".join(keys).encode()).hexdigest()[:16] == hashlib.sha256("\n".join(want).encode()).hexdigest()[:16] == KEYS_SHA
    assert [tuple(p.shape) for p in m.actor.parameters()] == [(64, 14), (64,), (64, 64), (64,), (4, 64), (4,)]
    assert m.net_arch == (64, 64) and m.activation == "tanh" and m.algo == "td3"
    assert all(not p.requires_grad for p in m.target_parameters()) and all(p.requires_grad for p in m.actor.parameters())
    assert all(torch.equal(a, b) for a, b in zip(m.target_parameters(), list(m.actor.parameters()) + m.critic_parameters()))
    # creation order: the same seed gives the same actor whatever follows it, and the critics draw after the actor
    torch.manual_seed(5)
    a = Td3Policy(14, 4)
    torch.manual_seed(5)
    first = torch.nn.Linear(14, 64)
    assert torch.equal(a.actor[0].weight, first.weight)
    with pytest.raises(ValueError):
        Td3Policy(14, 4, (), "tanh")
    with pytest.raises(ValueError):
        Td3Policy(14, 4, (64, 64), "gelu")


KEYS_SHA = hashlib.sha256("\n".join("%s.%d.%s" % (t, i, k) for t in ("actor", "q1", "q2", "actor_target", "q1_target", "q2_target") for i in (0, 2, 4)
                                    for k in ("weight", "bias")).encode()).hexdigest()[:16]


def _torch_batch(b):
    return {k: (None if b[k] is None else torch.from_numpy(b[k])) for k in ("obs", "next_obs", "action", "reward", "done", "use")}


def test_a_relu_128_128_module_runs_through_td3_step():
    from gym_xarm_amd.td3 import STATS, Td3Policy, make_optimizers, td3_step
    torch.manual_seed(0)
    m = Td3Policy(14, 4, (128, 128), "relu")
    opts = make_optimizers(m)
    b = _torch_batch(TH.make_batch(14, 4, 65))
    b = {k: v for k, v in b.items() if v is not None}
    last = None
    for n in (1, 2, 3):
        last = td3_step(m, opts, b, n, last=last)
        assert tuple(last.keys()) == STATS and all(v.dim() == 0 and bool(torch.isfinite(v)) for v in last.values())
        assert float(last["actor_stepped"]) == float(n % 2 == 0)
    assert float(last["actor_loss"]) == -float(last["q1_pi"]) != 0.0          # step 3 repeats step 2's


def test_checkpoint_round_trip_carries_shape_and_algo(tmp_path):
    from safetensors import safe_open
    from gym_xarm_amd import sac, td3
    from gym_xarm_amd.train import VecNormalize, save_model
    from test_sac_host import scripted_goal_env
    venv = VecNormalize(scripted_goal_env(4))
    m = td3.Td3Policy(venv.dim, 2, (128, 128, 128), "relu")
    path = str(tmp_path / "td3.safetensors")
    save_model(path, m, venv)
    with safe_open(path, framework="pt") as f:
        assert f.metadata() == {"net_arch": "128,128,128", "activation": "relu", "algo": "td3"}
    m2, vs = td3.load_checkpoint(path)
    assert m2.net_arch == (128, 128, 128) and m2.activation == "relu" and m2.act_dim == 2
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values())) and set(vs) == set(venv.state_dict())
    # an SAC checkpoint keeps its keys and metadata and still loads; td3.load_checkpoint refuses a file that names another algo
    s = sac.SacPolicy(venv.dim, 2, (128, 128), "relu")
    spath = str(tmp_path / "sac.safetensors")
    save_model(spath, s, venv)
    with safe_open(spath, framework="pt") as f:
        assert f.metadata() == {"net_arch": "128,128", "activation": "relu"}
        assert sorted(f.keys()) == sorted(["policy." + k for k in s.state_dict()] + ["vecnormalize." + k for k in venv.state_dict()])
    s2, _ = sac.load_checkpoint(spath)
    assert all(torch.equal(a, b) for a, b in zip(s.state_dict().values(), s2.state_dict().values()))


# ------------------------------------------------------------------------------------------------------- td3_step against float64
@pytest.mark.parametrize("policy_delay", (1, 2))
def test_td3_step_against_a_float64_copy(policy_delay):
    """the public block, float32, against td3_host's float64 restatement fed the same z: parameters after one step within 4 lr (Adam's
    first step is lr sign(g): an entry whose gradient rounds across zero lands 2 lr away), the per-row y within the block rule"""
    from gym_xarm_amd.td3 import make_optimizers, td3_step
    shape, B = TH.SHAPE_64, 65
    h = TH.hyper(policy_delay=policy_delay)
    model = TH.make_model(shape)
    b = TH.make_batch(shape[0], shape[1], B)
    for n in ((1,) if policy_delay == 1 else (1, 2)):
        m32 = copy.deepcopy(model)
        before = [p.detach().clone() for p in TH.model_tensors(m32)]
        st = td3_step(m32, make_optimizers(m32, h["lr"]), {k: v for k, v in _torch_batch(b).items() if v is not None}, n, h["gamma"], h["tau"],
                      policy_delay, h["target_policy_noise"], h["target_noise_clip"], z_next=torch.from_numpy(b["z_next"]))
        m64, _, r64 = TH.torch_steps(model, [b], h, torch.float64, first=n)
        stepped = n % policy_delay == 0
        assert float(st["actor_stepped"]) == float(stepped) and float(st["n_use"]) == r64[0]["stats"]["n_use"]
        for k in ("critic_loss", "target_q") + (("actor_loss", "q1_pi") if stepped else ()):
            assert float(st[k]) == pytest.approx(r64[0]["stats"][k], rel=1e-4, abs=1e-5), k
        assert np.abs(TH.model_flat(m32) - TH.model_flat(m64)).max() <= 4 * h["lr"]
        assert np.abs(TH.model_flat(m32, "targets") - TH.model_flat(m64, "targets")).max() <= 1e-5
        tp = len(before) // 6
        same = [torch.equal(a, p) for a, p in zip(before, TH.model_tensors(m32))]
        if stepped:
            assert not any(same)
        else:       # the actor, its target and the critics' targets are bitwise untouched; the critics moved
            assert all(same[:tp]) and all(same[3 * tp:]) and not any(same[tp:3 * tp])
            assert float(st["actor_loss"]) == 0.0 and float(st["q1_pi"]) == 0.0


# ------------------------------------------------------------------------------------------------------ host build against float64
@pytest.mark.parametrize("case", TH.CASES, ids=TH.case_id)
def test_host_step_against_float64(case):
    shape, B = case
    ref = TH.reference(shape, B)
    w, m, v, step = TH.ref_state(ref)
    rc, out = TH.host_update(w, m, v, step, ref["b"], ref["h"], shape)
    assert rc == TH.geometry(B, shape)["launches"] == 7 * shape[3] + 14 and step[0] == ref["step"] + 1
    fig = TH.check_step(out, ref, TH.case_id(case))
    print("%s: Y %.2e, settled out %d rows, figures in Y %s" % (TH.case_id(case), ref["Y"], ref["lost"], {k: round(float(x), 2) for k, x in fig.items()}))
    used = int((ref["r64"]["use"] != 0).sum())
    assert used >= 1 and ref["lost"] <= 0.2 * B
    parts = TH.work_parts(out["work"], B, shape)
    assert parts["flag"] == 0 and np.array_equal(parts["y"], out["y"]) and np.abs(parts["a_next"]).max() <= 1.0
    assert np.abs(parts["a_pi"] - ref["r64"]["a_pi"]).max() <= 1e-5 and np.abs(parts["a_next"] - ref["r64"]["a_next"]).max() <= 1e-5


def test_a_delayed_step_against_float64():
    """step 1 of policy_delay 2: the critics' gradients under the rule; the actor's gradient, dq1/da and the actor phase's stats untouched"""
    shape, B = A_, 200
    ref = TH.reference(shape, B, policy_delay=2, n_updates=1)
    w, m, v, step = TH.ref_state(ref)
    w0 = [a.copy() for a in w]
    stats = np.array([9, 3, 4, 9, 9, 9, 9, 9], np.float32)
    rc, out = TH.host_update(w, m, v, step, ref["b"], ref["h"], shape, stats=stats)
    assert rc == 7 * shape[3] + 14
    TH.check_step(dict(out, stats=np.array([out["stats"][0], 0, 0] + list(out["stats"][3:]), np.float32)), ref, "delayed")
    assert out["stats"][1] == 3.0 and out["stats"][2] == 4.0 and out["stats"][5] == 0.0
    tp = len(w) // 6
    assert all(np.array_equal(a, c) for a, c in zip(w0[:tp] + w0[3 * tp:], w[:tp] + w[3 * tp:])) and not any(np.array_equal(a, c) for a, c in zip(w0[tp:3 * tp], w[tp:3 * tp]))
    assert not out["grad"][:TH.geometry(B, shape)["Pa"]].any() and not out["dqda"].any() and TH.work_parts(out["work"], B, shape)["flag"] == 1


def test_4097_rows_cover_every_row_range():
    """16 row ranges and a one-row tile; lr = 0 so that the stepped q1 is the call's own"""
    shape, B = (14, 4, 64, 2, "relu"), 4097
    geo = TH.geometry(B, shape)
    assert geo["S"] == 16 and geo["rows"][-1] == B and geo["rows"][16] - geo["rows"][15] == 257 and B % 32 == 1
    ref = TH.reference(shape, B, lr=0.0)
    w, m, v, step = TH.ref_state(ref)
    rc, out = TH.host_update(w, m, v, step, ref["b"], ref["h"], shape)
    assert rc > 0
    TH.check_step(out, ref, "4097 rows")


# --------------------------------------------------------------------------------------------------------------------- whole steps
def host_runner(shape, record=None):
    def run(model, batches, h):
        w, m, v, step = TH.fresh_state(model)
        stats = np.zeros(8, np.float32)
        for b in batches:
            rc, out = TH.host_update(w, m, v, step, b, h, shape, stats=stats)
            assert rc > 0
            if record is not None:
                record.append((copy.deepcopy(w), stats.copy()))
        assert step[0] == len(batches)
        return TH.flat_of(TH.trained_of(w)), TH.flat_of(w[len(w) // 2:])
    return run


@pytest.mark.parametrize("shape,policy_delay,n_steps", [(A_, 2, 4), (A_, 1, 3), (REF, 2, 4), (REF, 1, 3)], ids=["A-delay2", "A-delay1", "REF-delay2", "REF-delay1"])
def test_whole_steps_against_float64(shape, policy_delay, n_steps):
    cap = 0.01 if shape == A_ else min(0.08, 1.25 * REF_MEASURED[policy_delay])
    rec = []
    res, Y, share, worst_t = TH.parameter_case(shape, 200, n_steps, policy_delay, host_runner(shape, rec), cap)
    print("whole steps %s delay %d: Y %.2e, left out %.3f %% (cap %.3f %%), rule %s, targets %.2f" %
          (shape, policy_delay, Y, 100 * share, 100 * cap, {k: round(v[0], 2) for k, v in res.items()}, worst_t))
    for k, (worst, in_y) in res.items():
        assert worst <= 1.0, "%s parameters %.2f x their bound (%.1f Y)" % (k, worst, in_y)
    assert worst_t <= 1.0
    # the delay: the actor and every target move on the calls whose count is a multiple of policy_delay and on no other
    tp = len(rec[0][0]) // 6
    prev = TH.weights_of(TH.make_model(shape))
    for i, (w, stats) in enumerate(rec):
        stepped = (i + 1) % policy_delay == 0
        same = [np.array_equal(a, c) for a, c in zip(prev, w)]
        assert (not any(same[:tp] + same[3 * tp:])) if stepped else all(same[:tp] + same[3 * tp:]), i
        assert not any(same[tp:3 * tp]) and stats[5] == float(stepped)
        prev = w


# what the torch float32 / float64 pair alone leaves out of a tensor at SHAPE_REF, B = 200 - the largest share over seeds 0 .. 3, measured
# with td3_host.left_out on the CPU (four steps at policy_delay 2, three at policy_delay 1).  The asserted cap is this plus a quarter, and
# never above sacw's 8 %
REF_MEASURED = {2: 0.0354, 1: 0.0105}        # seeds 0 .. 3: 0.98, 1.03, 3.54, 1.40 % and 0.63, 0.56, 0.68, 1.05 %


# ------------------------------------------------------------------------------------------------------------------- smaller cases
def test_an_all_masked_batch_changes_nothing_but_the_step():
    shape, B = A_, 65
    model = TH.make_model(shape)
    b = dict(TH.make_batch(shape[0], shape[1], B), use=np.zeros(B, np.float32))
    w, m, v, step = TH.fresh_state(model)
    w0 = [a.copy() for a in w]
    rc, out = TH.host_update(w, m, v, step, b, TH.hyper(policy_delay=1), shape)
    assert rc > 0 and step[0] == 1 and out["stats"][4] == 1.0 and out["stats"][0] == 0.0        # n_use = max(0, 1)
    tp = len(w) // 6
    assert all(np.array_equal(a, c) for a, c in zip(w0[:3 * tp], w[:3 * tp])) and not any(a.any() for a in m + v)
    assert all(np.isfinite(a).all() for a in w) and np.isfinite(out["stats"]).all() and np.isfinite(out["y"]).all() and not out["grad"].any()


def test_given_noise_and_philox_noise():
    shape, B = A_, 65
    model = TH.make_model(shape)
    b = TH.make_batch(shape[0], shape[1], B)
    h = TH.hyper(policy_delay=1)
    run = lambda noise, **kw: TH.host_update(*TH.fresh_state(model, kw.pop("step", 0)), b, dict(h, **kw), shape, noise=noise)[1]
    given, ph, ph2 = run(True), run(False), run(False)
    assert np.array_equal(ph["y"], ph2["y"]) and not np.array_equal(ph["y"], given["y"])                # repeatable, and not the given draw
    assert not np.array_equal(ph["y"], run(False, seed=1)["y"]) and not np.array_equal(ph["y"], run(False, step=2)["y"])
    a_ph = TH.work_parts(ph["work"], B, shape)["a_next"]
    a0 = TH.work_parts(run(False, target_policy_noise=0.0)["work"], B, shape)["a_next"]
    assert np.abs(a_ph - a0).max() <= 0.5 + 1e-6 and 0.05 < np.abs(a_ph - a0).std() < 0.3              # sigma 0.2, clipped at 0.5
    # a row's draw is keyed by row_offset + row: row 3 at offset 0 is row 0 at offset 3
    b1 = {k: (None if x is None else np.ascontiguousarray(x[3:4])) for k, x in b.items()}
    one = TH.host_update(*TH.fresh_state(model), b1, h, shape, noise=False, row_offset=3)[1]
    assert np.array_equal(TH.work_parts(one["work"], 1, shape)["a_next"][0], a_ph[3])


def test_clip_edge_zero_clip_is_the_plain_target_action():
    shape, B = A_, 65
    model = TH.make_model(shape)
    b = TH.make_batch(shape[0], shape[1], B)
    out = TH.host_update(*TH.fresh_state(model), b, TH.hyper(policy_delay=1, target_noise_clip=0.0), shape)[1]
    w = TH.weights_of(model)
    tp = len(w) // 6
    det = TH.host_act(w[3 * tp:4 * tp] + w[tp:], b["next_obs"], shape, TH.hyper())                    # actor_target in the actor's place
    assert np.array_equal(TH.work_parts(out["work"], B, shape)["a_next"], np.clip(det, -1.0, 1.0))


def test_optimiser_state_hand_over_in_both_directions():
    """two torch steps, then a host-build step from the exported state, against three torch steps - and back"""
    shape, B = TH.SHAPE_64, 65
    h = TH.hyper(policy_delay=2)
    model = TH.make_model(shape)
    batches = [TH.make_batch(shape[0], shape[1], B, seed=s) for s in range(3)]
    m64 = TH.torch_steps(model, batches, h, torch.float64)[0]
    m32, opts, _ = TH.torch_steps(model, batches[:2], h, torch.float32)
    ps = TH.trained_of(TH.model_tensors(m32))
    tp = len(ps) // 3
    steps = {k: {int(opts[k].state[p]["step"]) for p in ps[sl]} for k, sl in (("actor", slice(0, tp)), ("critic", slice(tp, 3 * tp)))}
    assert steps == {"actor": {2 // 2}, "critic": {2}}                  # the actor count is step // policy_delay
    w = TH.weights_of(m32)
    state = lambda key: [PH.aligned(opts["actor" if i < tp else "critic"].state[p][key].numpy().copy()) for i, p in enumerate(ps)]
    m, v, step = state("exp_avg"), state("exp_avg_sq"), np.full(1, 2, np.int64)
    rc, out = TH.host_update(w, m, v, step, batches[2], h, shape)
    assert rc > 0 and step[0] == 3 and out["stats"][5] == 0.0
    sz, grp = TH.sizes(model), TH.groups(model)
    m32b, opts_b, _ = TH.torch_steps(model, batches, h, torch.float32)
    p64, p32 = TH.model_flat(m64), TH.model_flat(m32b)
    Y = WH.yardstick(p32, p64, sz)
    for k, (worst, in_y) in WH.rule(TH.flat_of(TH.trained_of(w)), p64, max(Y, 2.0 ** -24), sz, grp).items():
        assert worst <= 1.0, (k, worst, in_y)
    # and back: torch Adams continue from the host build's state - the critics' at step 3, the actor's at 3 // 2 - through step 4
    m4 = copy.deepcopy(model)
    with torch.no_grad():
        for t, a in zip(TH.model_tensors(m4), w):
            t.copy_(torch.from_numpy(a))
    o4 = TH.make_opts(m4, h)
    for i, p in enumerate(TH.trained_of(TH.model_tensors(m4))):
        o4["actor" if i < tp else "critic"].state[p] = {"step": torch.tensor(float(3 // 2 if i < tp else 3)), "exp_avg": torch.from_numpy(m[i].copy()),
                                                        "exp_avg_sq": torch.from_numpy(v[i].copy())}
    b4 = TH.make_batch(shape[0], shape[1], B, seed=3)
    TH.torch_step(m4, o4, b4, h, 4)
    p64 = TH.model_flat(TH.torch_steps(model, batches + [b4], h, torch.float64)[0])
    p32 = TH.model_flat(TH.torch_steps(model, batches + [b4], h, torch.float32)[0])
    for k, (worst, in_y) in WH.rule(TH.model_flat(m4), p64, max(WH.yardstick(p32, p64, sz), 2.0 ** -24), sz, grp).items():
        assert worst <= 1.0, (k, worst, in_y)
    assert int(o4["actor"].state[TH.trained_of(TH.model_tensors(m4))[0]]["step"]) == 2 and int(o4["critic"].state[TH.trained_of(TH.model_tensors(m4))[tp]]["step"]) == 4


def test_the_library_refuses_bad_arguments_before_any_launch():
    """every XARM_E_INVALID case through libxarm_hip.so itself and through the host build: the checks come before any launch, so this runs
    without a GPU"""
    from gym_xarm_amd import _native
    L = _native.load()
    shape, B = REF, 65
    D, A, H, NL, _ = shape
    b = TH.make_batch(D, A, B)
    w, m, v, step = TH.fresh_state(TH.make_model(shape))
    work = TH.workspace(B, shape)
    calls, out_a = np.zeros(1, np.int64), np.zeros((B, A), np.float32)
    P = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    lay = lambda **kw: _native.XarmSACWLayout(**dict(dict(batch_size=B, obs_dim=D, act_dim=A, hidden=H, n_hidden=NL, activation=1, row_offset=0), **kw))

    def update(layout=None, edit=None, null=(), work_ptr="ok", mode="deterministic", **hy):
        S = [TH.abi_weights(w), TH.abi_weights(m), TH.abi_weights(v)]
        if edit:
            edit(S)
        data = {k: (None if k in null else P(b[k])) for k in ("obs", "next_obs", "action", "reward", "done", "use")}
        wk = {"ok": P(work), "null": None, "odd": C.c_void_p(work.ctypes.data + 4)}[work_ptr]
        args = [C.byref(layout or lay()), C.byref(TH.abi_params(TH.hyper(**hy), mode))] + [C.byref(s) for s in S] + \
               [None if "step" in null else P(step), data["obs"], data["next_obs"], data["action"], data["reward"], data["done"], data["use"], None, wk,
                None, None, None, None, None]
        return L.xarm_td3_update(*args, None), min(TH.lib().t3h_update(*args), 0)

    def act(layout=None, edit=None, null=(), work_ptr="ok", mode="gaussian", **hy):
        S = [TH.abi_weights(w)]
        if edit:
            edit(S)
        wk = {"ok": P(work), "null": None, "odd": C.c_void_p(work.ctypes.data + 4)}[work_ptr]
        params = TH.abi_params(TH.hyper(**hy), mode if isinstance(mode, str) else "deterministic")
        if not isinstance(mode, str):
            params.mode = mode
        args = [C.byref(layout or lay()), C.byref(params), C.byref(S[0]), None if "calls" in null else P(calls),
                None if "obs" in null else P(b["obs"]), wk, None if "action" in null else P(out_a)]
        return L.xarm_td3_act(*args, None), TH.lib().t3h_act(*args)

    # every layout xarm_sacw_* refuses
    for kw in (dict(hidden=96), dict(hidden=320), dict(n_hidden=1), dict(n_hidden=4), dict(activation=2), dict(act_dim=9), dict(obs_dim=89, act_dim=8),
               dict(obs_dim=93, act_dim=4), dict(batch_size=-1), dict(obs_dim=0), dict(row_offset=-1), dict(hidden=0), dict(activation=-1)):
        assert update(layout=lay(**kw)) == (-1, -1) and b"xarm_td3_update" in L.xarm_last_error(None), kw
        assert act(layout=lay(**kw)) == (-1, -1) and b"xarm_td3_act" in L.xarm_last_error(None), kw
        n = C.c_int64(-5)
        assert L.xarm_td3_workspace_bytes(C.byref(lay(**kw)), C.byref(n)) == -1 and TH.lib().t3h_workspace_bytes(C.byref(lay(**kw))) == -1
    # TD3's own: policy_delay < 1, a negative noise or clip, tau outside [0, 1] - and the hyper-parameters xarm_sacw_update refuses
    for hy, word in ((dict(policy_delay=0), b"policy_delay"), (dict(policy_delay=-2), b"policy_delay"), (dict(target_policy_noise=-0.1), b"target_policy_noise"),
                     (dict(target_noise_clip=-0.5), b"target_noise_clip"), (dict(action_noise=-1.0), b"action_noise"), (dict(tau=1.5), b"tau"),
                     (dict(tau=-0.1), b"tau"), (dict(target_policy_noise=float("nan")), b"target_policy_noise"), (dict(gamma=1.5), b"gamma"),
                     (dict(lr=-1.0), b"lr"), (dict(beta1=1.0), b"beta"), (dict(eps=0.0), b"eps")):
        assert update(**hy) == (-1, -1) and word in L.xarm_last_error(None), hy
    assert act(policy_delay=0) == (-1, -1) and act(mode=3) == (-1, -1) and b"mode" in L.xarm_last_error(None)

    def misalign(S):
        S[0].q1[2] = w[2 * (NL + 1) + 2].ctypes.data + 4

    def null_tensor(S):
        S[0].actor_target[3] = None

    def null_state(S):
        S[1].actor[0] = None
    assert update(edit=misalign) == (-1, -1) and b"aligned" in L.xarm_last_error(None)
    assert update(edit=null_tensor) == (-1, -1) and update(edit=null_state) == (-1, -1)
    for k in ("obs", "next_obs", "action", "reward", "done", "step"):
        assert update(null=(k,)) == (-1, -1), k
    assert update(work_ptr="null") == (-1, -1) and update(work_ptr="odd") == (-1, -1)

    def act_null(S):
        S[0].actor[2 * NL + 1] = None
    assert act(edit=act_null) == (-1, -1)
    for k in ("calls", "obs", "action"):
        assert act(null=(k,)) == (-1, -1), k
    assert act(work_ptr="null") == (-1, -1) and act(work_ptr="odd") == (-1, -1)
    # batch_size == 0 launches nothing and returns OK whatever the pointers are
    assert update(layout=lay(batch_size=0), null=("obs", "next_obs", "action", "reward", "done", "step"), work_ptr="null") == (0, 0)
    assert act(layout=lay(batch_size=0), null=("calls", "obs", "action"), work_ptr="null") == (0, 0)
    n = C.c_int64(-5)
    assert L.xarm_td3_workspace_bytes(C.byref(lay()), C.byref(n)) == 0 and n.value > 0 and n.value % 16 == 0
    assert n.value == TH.lib().t3h_workspace_bytes(C.byref(lay()))
    geo = TH.geometry(B, shape)
    assert geo["launches"] == 7 * NL + 14 and geo["act_launches"] == NL + 2 and TH.lib().t3h_param_count(C.byref(lay())) == sum(TH.sizes(TH.make_model(shape)))
    assert TH.geometry(65536, shape)["S"] == 16 == TH.geometry(4097, shape)["S"] and TH.geometry(256, shape)["S"] == 4


def test_host_act_modes():
    shape = A_
    model = TH.make_model(shape)
    w = TH.weights_of(model)
    obs = TH.make_batch(shape[0], shape[1], 200)["obs"]
    h = TH.hyper()
    det = TH.host_act(w, obs, shape, h)
    with torch.no_grad():
        assert np.abs(det - model.action(torch.from_numpy(obs)).numpy()).max() <= 1e-5
    calls = np.full(1, 7, np.int64)
    g = TH.host_act(w, obs, shape, h, "gaussian", calls)
    u = TH.host_act(w, obs, shape, h, "uniform", calls)
    assert calls[0] == 9 and np.abs(g).max() <= 1.0 and 0.05 < (g - det).std() < 0.15 and -1.0 <= u.min() < -0.9 and 0.9 < u.max() <= 1.0 and abs(u.mean()) < 0.1
    # a row does not depend on its batch: rows 31 .. 64 alone at row_offset 31
    for mode in ("deterministic", "gaussian", "uniform"):
        whole = TH.host_act(w, obs, shape, h, mode, np.full(1, 7, np.int64))
        part = TH.host_act(w, np.ascontiguousarray(obs[31:65]), shape, h, mode, np.full(1, 7, np.int64), row_offset=31)
        assert np.array_equal(whole[31:65], part), mode


def test_device_class_names_the_limit_and_the_path_that_runs():
    from gym_xarm_amd.device_td3 import DeviceTD3
    from gym_xarm_amd.td3 import Td3Policy
    for arch, word in (((400, 300), "same width"), ((256, 256, 256, 256), "two or three"), ((512, 512), "64, 128, 192 or 256")):
        with pytest.raises(ValueError, match=word) as e:
            DeviceTD3(Td3Policy(14, 4, arch, "relu"), 256)
        assert "td3_step" in str(e.value)
    with pytest.raises(ValueError, match="torch block of train_td3"):
        DeviceTD3(Td3Policy(14, 4, (256, 256, 256), "relu"), 256)
    with pytest.raises(ValueError, match="torch block of train_td3"):
        DeviceTD3(Td3Policy(14, 4), 256)


# ----------------------------------------------------------------------------------------------------------------------- driver
def test_train_td3_runs_a_relu_net_on_the_scripted_env():
    from test_sac_host import scripted_goal_env
    from gym_xarm_amd.td3 import STATS, train_td3
    model, venv, hist = train_td3(env_id="Scripted-v0", env=scripted_goal_env(16), steps=40, batch_size=32, quiet=True, log_every=20, seed=0,
                                  net_arch=(128, 128), activation="relu")
    assert model.net_arch == (128, 128) and model.activation == "relu" and isinstance(model.q1[1], torch.nn.ReLU)
    assert len(hist) == 2 and hist[-1]["updates"] == 28 and hist[-1]["env_steps"] == 40 * 16 and set(STATS) <= set(hist[-1])
    for rec in hist:
        assert all(np.isfinite(x) for x in rec.values()), rec
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters()) and hist[-1]["actor_stepped"] == 1.0 and hist[-1]["actor_loss"] != 0.0
    for name in ("actor", "q1", "q2"):
        assert not torch.equal(getattr(model, name + "_target")[0].weight, getattr(model, name)[0].weight)
    with pytest.raises(ValueError, match="torch block of train_td3"):
        train_td3(env_id="Scripted-v0", env=scripted_goal_env(16), steps=2, quiet=True, device_update=True)


def test_the_shared_driver_loop_keeps_train_sac_bit_for_bit():
    """train_sac moved its loop into sac.train_off_policy: for a fixed seed its history equals the one recorded before the move
    (tests/golden/sac_scripted_hist.json), in every field but the wall-clock rate"""
    from test_sac_host import scripted_goal_env
    from gym_xarm_amd.sac import train_sac
    with open(os.path.join(PH.ROOT, "tests", "golden", "sac_scripted_hist.json")) as f:
        gold = json.load(f)
    a = gold["args"]
    model, venv, hist = train_sac(env_id="Scripted-v0", env=scripted_goal_env(a["num_envs"]), steps=a["steps"], batch_size=a["batch_size"], quiet=True,
                                  log_every=a["log_every"], seed=a["seed"])
    for rec in hist:
        assert rec.pop("env_steps_per_sec") > 0
    assert hist == gold["hist"]


def test_cli_dispatches_td3(monkeypatch):
    import gym_xarm_amd.sac as sac
    import gym_xarm_amd.td3 as td3
    import gym_xarm_amd.train as tr
    seen = {}
    monkeypatch.setattr(td3, "train_td3", lambda *a, **kw: seen.update(td3=(a, kw)) or (None, None, []))
    monkeypatch.setattr(sac, "train_sac", lambda *a, **kw: seen.update(sac=(a, kw)) or (None, None, []))
    monkeypatch.setattr("sys.argv", ["train", "--algo", "td3", "--env", "XarmReach-v0", "--num-envs", "64", "--updates", "100", "--batch-size", "128",
                                     "--gradient-steps", "2", "--device-update", "--device-normalize", "--reward-type", "sparse", "--net-arch", "256", "256", "256",
                                     "--activation", "relu", "--policy-delay", "3", "--target-policy-noise", "0.3", "--target-noise-clip", "0.6",
                                     "--action-noise", "0.2"])
    tr.main()
    a, kw = seen["td3"]
    assert "sac" not in seen and kw["batch_size"] == 128 and kw["gradient_steps"] == 2 and kw["device_update"] is True and kw["device_normalize"] is True
    assert kw["steps"] == 100 and kw["num_envs"] == 64 and kw["config"]["reward_type"] == "sparse" and kw["net_arch"] == (256, 256, 256)
    assert kw["activation"] == "relu" and kw["policy_delay"] == 3 and kw["target_policy_noise"] == 0.3 and kw["target_noise_clip"] == 0.6 and kw["action_noise"] == 0.2
    monkeypatch.setattr("sys.argv", ["train", "--algo", "td3"])
    tr.main()
    assert "policy_delay" not in seen["td3"][1] and seen["td3"][1]["net_arch"] is None            # train_td3's own defaults
    for argv in (["--algo", "sac", "--policy-delay", "2"], ["--algo", "ppo", "--action-noise", "0.1"], ["--algo", "td3", "--target-kl", "0.1"],
                 ["--algo", "td3", "--lr-schedule", "linear"], ["--algo", "td3", "--wide"], ["--algo", "td3", "--shuffle", "device"]):
        monkeypatch.setattr("sys.argv", ["train"] + argv)
        with pytest.raises(SystemExit):
            tr.main()


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
    """steps and act calls over the shapes and row counts of these tests through the host core as a stand-alone program (its own main,
    never loaded into python)"""
    exe = str(tmp_path / "td3_main_san")
    src = os.path.join(TH.DIR, "td3_main.cpp")
    subprocess.check_call(["g++", "-g"] + WH.gxx_flags() + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                            "-fno-omit-frame-pointer", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "td3_main ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
