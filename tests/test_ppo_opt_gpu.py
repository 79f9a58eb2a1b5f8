"""The PPO options - clip_range_vf and the device-side target_kl stop (include/xarm_hip.h xarm_ppo_options) - through
DevicePPO on the GPU.  The wide backend is held to the BITS of its host build (tests/hostbuild_ppo_opt); the fused tile, whose sums
over rows run in another order than its host build's, to train.py's torch block in float64 under the parameter rule and check_stats's
bounds, with the stop's step exact.  Then the options that never act, run-to-run bits, a captured update that stops, and train().
Cases and their validity conditions: tests/ppo_opt_host.py; the CPU side: tests/test_ppo_opt_host.py."""
import numpy as np
import pytest
import torch

import policy_host as PH
import ppo_host as PP
import ppo_opt_host as O
import ppow_host as W

pytestmark = pytest.mark.gpu


def device_ppo(c, **kw):
    from gym_xarm_amd.device_ppo import DevicePPO
    model = O.model_of(c).cuda()
    ppo = DevicePPO(model, c[4], n_steps=c[3], n_epochs=c[6], batch_size=c[5], lr=O.LR, wide=True if c[0] == "wide" else None, **kw)
    assert ppo.backend == ("wide" if c[0] == "wide" else "tile64")
    return model, ppo


def fill(ppo, b, perm):
    for k in ("obs", "action", "reward", "done", "use"):
        ppo.buffers[k].copy_(torch.from_numpy(b[k]))
    ppo.perm.copy_(torch.from_numpy(perm))
    return torch.from_numpy(b["last_obs"]).cuda()


def dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def device_arrays(ppo):
    """what state_arrays walks on the host side, from the device, and the stats"""
    return [t.detach().cpu().numpy() for t in list(ppo.params()) + ppo.exp_avg + ppo.exp_avg_sq + [ppo.step]] + [ppo.stats.cpu().numpy()]


def run(c, old_logp=None, b=None, **kw):
    model, ppo = device_ppo(c, **kw)
    ppo.update(fill(ppo, O.batch_of(c) if b is None else b, O.perm_of(c)), shuffle=False, old_logp=dev(old_logp))
    return ppo


def flat_params(ppo):
    return np.concatenate([p.detach().cpu().numpy().astype(np.float64).ravel() for p in ppo.params()])


# ------------------------------------------------------------------------------------------------------------------- wide backend
@pytest.mark.parametrize("c", O.WIDE, ids=O.case_id)
def test_wide_backend_with_the_options_equals_its_host_build(c):
    """each option alone, both together (old_logp computed at call start, the stop inside an epoch), and a stop at step 0 with a supplied
    old_logp: weights, Adam state, step and stats bit for bit the host build's"""
    s = O.SETTINGS[c]
    h = PP.hyper(lr=O.LR)
    spread = PP.spread_old_logp(O.model_of(c), O.batch_of(c), h)
    stops = []
    for kw, olp in ((dict(clip_range_vf=s["c_vf"]), spread), (dict(target_kl=s["mid"]), None), (dict(clip_range_vf=s["c_vf"], target_kl=s["mid"]), None),
                    (dict(target_kl=0.02), spread)):
        ppo = run(c, olp, **kw)
        state = O.fresh_state(c)
        rc, out = O.host_update(c, state, h, O.perm_of(c), olp, O.options(**kw))
        assert rc == 0 and O.same_bits(device_arrays(ppo), O.state_arrays(c, state) + [out["stats"]]), kw
        stops.append(int(ppo.step[0]))
        assert ppo.steps_applied() == stops[-1]
    S = O.steps_of(c)
    assert stops[0] == S and 1 <= stops[1] <= S - 2 and 1 <= stops[2] <= S - 2 and stops[3] == 0, stops


@pytest.mark.parametrize("c", O.TILE + O.WIDE, ids=O.case_id)
def test_options_that_never_act_are_invisible_on_the_device(c):
    """clip_range_vf = target_kl = 1e30 against no options: every bit of weights, Adam state, step, stats, adv, returns and step 0's
    gradient; and a second identical call with the options gives the same bits again"""
    runs = []
    for kw in ({}, dict(clip_range_vf=1e30, target_kl=1e30), dict(clip_range_vf=1e30, target_kl=1e30)):
        model, ppo = device_ppo(c, ent_coef=0.01, **kw)
        T, E = c[3], c[4]
        outs = [torch.full((T, E), float("nan"), device="cuda"), torch.full((T, E), float("nan"), device="cuda"), torch.full((ppo.num_params,), float("nan"), device="cuda")]
        ppo.update(fill(ppo, O.batch_of(c), O.perm_of(c)), shuffle=False, out_adv=outs[0], out_returns=outs[1], out_grad=outs[2])
        runs.append(device_arrays(ppo) + [x.cpu().numpy() for x in outs])
        assert int(ppo.step[0]) == O.steps_of(c)
    assert all(np.isfinite(x).all() for x in runs[0]) and O.same_bits(runs[0], runs[1]) and O.same_bits(runs[1], runs[2])


# --------------------------------------------------------------------------------------------------------------------- fused tile
@pytest.mark.parametrize("c", O.TILE, ids=O.case_id)
def test_fused_tile_value_clip_against_float64(c):
    c_vf = O.SETTINGS[c]["c_vf"]
    r = O.reference(c, "spread", clip_range_vf=c_vf)
    O.assert_valid_clip(r["r64"]["recs"], r["h"], c_vf)
    runs = [run(c, r["old_logp"], clip_range_vf=c_vf) for _ in range(2)]
    assert O.same_bits(device_arrays(runs[0]), device_arrays(runs[1]))                       # two identical calls, identical bits
    ppo = runs[0]
    assert int(ppo.step[0]) == O.steps_of(c) and bool((ppo.stats[:, 7] == 0).all())
    ratio, in_y, Y, left = O.parameter_rule(c, r, flat_params(ppo))
    print("device PPO with clip_range_vf %g, %s: parameters after %d steps: Y %.2e, error %.2f Y, error / bound %.3f, left out %d"
          % (c_vf, O.case_id(c), O.steps_of(c), Y, in_y, ratio, left))
    assert ratio <= 1.0
    O.check_rows(c, r, ppo.stats.cpu().numpy())
    plain = run(c, r["old_logp"])
    assert not O.same_bits(device_arrays(plain)[:13], device_arrays(ppo)[:13])                # the clip is not a no-op here


@pytest.mark.parametrize("which,old_logp", (("mid", None), ("epoch", None), ("zero", "spread")))
@pytest.mark.parametrize("c", O.TILE, ids=O.case_id)
def test_fused_tile_kl_stop_against_float64(c, which, old_logp):
    """the tripping step, `step` and stats[:, 7] exact under assert_valid_stop's margin; parameters by the rule, stats rows by their bounds;
    nothing applied past the stop: Adam's state equals that of a device call with as many epochs as were completed, where the stop falls
    on an epoch's first step"""
    kl = 0.02 if which == "zero" else O.SETTINGS[c][which]
    r = O.reference(c, old_logp, target_kl=kl)
    s_star = O.assert_valid_stop(r, kl, c[2])
    S, M = O.steps_of(c), O.steps_of(c) // c[6]
    g = torch.full((sum(r["sizes"]),), float("nan"), device="cuda")
    model, ppo = device_ppo(c, target_kl=kl)
    ppo.update(fill(ppo, O.batch_of(c), r["perm"]), shuffle=False, old_logp=dev(r["old_logp"]), out_grad=g)
    again = run(c, r["old_logp"], target_kl=kl)
    assert O.same_bits(device_arrays(ppo), device_arrays(again))
    st = ppo.stats.cpu().numpy()
    assert int(ppo.step[0]) == s_star == ppo.steps_applied() and st[:, 7].tolist() == [0.0] * s_star + [1.0] * (S - s_star)
    assert (which, s_star == 0, s_star % M == 0) in (("mid", False, False), ("epoch", False, True), ("zero", True, True))
    O.check_rows(c, r, st)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0                       # step 0's gradient, also when step 0 trips
    if s_star == 0:
        assert O.same_bits(device_arrays(ppo)[:39], O.state_arrays(c, O.fresh_state(c))[:39])
        return
    ratio, in_y, Y, left = O.parameter_rule(c, r, flat_params(ppo))
    print("device PPO with target_kl %g, %s: trips at step %d of %d; parameters: Y %.2e, error %.2f Y, error / bound %.3f, left out %d"
          % (kl, O.case_id(c), s_star, S, Y, in_y, ratio, left))
    assert ratio <= 1.0
    if s_star % M == 0:
        from gym_xarm_amd.device_ppo import DevicePPO
        m2 = O.model_of(c).cuda()
        cut = DevicePPO(m2, c[4], n_steps=c[3], n_epochs=s_star // M, batch_size=c[5], lr=O.LR)
        for k in ("obs", "action", "reward", "done", "use"):
            cut.buffers[k].copy_(torch.from_numpy(O.batch_of(c)[k]))
        cut.perm.copy_(torch.from_numpy(r["perm"][:s_star // M]))
        cut.update(torch.from_numpy(O.batch_of(c)["last_obs"]).cuda(), shuffle=False)
        assert O.same_bits(device_arrays(ppo)[:40], device_arrays(cut)[:40])


def test_fused_tile_with_both_options():
    c = O.TILE[0]
    c_vf, kl = O.SETTINGS[c]["c_vf"], O.SETTINGS[c]["epoch"]
    r = O.reference(c, None, clip_range_vf=c_vf, target_kl=kl)
    s_star = O.assert_valid_stop(r, kl, c[2])
    ppo = run(c, None, clip_range_vf=c_vf, target_kl=kl)
    assert int(ppo.step[0]) == s_star >= 1
    O.check_rows(c, r, ppo.stats.cpu().numpy())
    assert O.parameter_rule(c, r, flat_params(ppo))[0] <= 1.0
    # grad() passes the options through and leaves the module and `step` alone
    before = [p.detach().clone() for p in ppo.params()]
    g, adv, ret, st = ppo.grad(torch.from_numpy(O.batch_of(c)["last_obs"]).cuda())
    assert int(ppo.step[0]) == s_star and all(torch.equal(p, q) for p, q in zip(ppo.params(), before)) and bool(torch.isfinite(g).all())
    assert bool((st[:, 7] == 0).all())                                                      # lr = 0: nothing moves, nothing trips


# -------------------------------------------------------------------------------------------------------------------------- graph
@pytest.mark.parametrize("c", (O.TILE[0], O.WIDE[0]), ids=O.case_id)
def test_captured_update_that_stops_replays_as_eager_updates(c):
    """an update with target_kl captured in a torch.cuda.graph; two replays on two batches against two eager calls on a twin, bit for
    bit.  The first call stops at step 3, the second, on other rows, at a later step (the host build: 7 and 5): each replay starts from
    a flag that the device cleared"""
    kind, D, A, T, E = c[:5]
    kl = 0.02
    b2 = PP.make_batch(D, A, T, E, 1.0, seed=2) if kind == "tile" else W.make_batch(O.shape_of(c), T, E, seed=2)
    batches, perm = [O.batch_of(c), b2], O.perm_of(c)
    model_g, ppo_g = device_ppo(c, target_kl=kl)
    model_e, ppo_e = device_ppo(c, target_kl=kl)
    last = torch.zeros(E, D, device="cuda")
    fill(ppo_g, batches[0], perm)
    ppo_g.grad(last)                             # the kernels are loaded before the capture; the module is not touched
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ppo_g.update(last, shuffle=False)
    stats_g, stats_e, steps = [], [], []
    for b in batches:
        last.copy_(fill(ppo_g, b, perm))
        graph.replay()
        stats_g.append(ppo_g.stats.clone())
        ppo_e.update(fill(ppo_e, b, perm), shuffle=False)
        stats_e.append(ppo_e.stats.clone())
        steps.append(int((stats_e[-1][:, 7] == 0).sum()))
    torch.cuda.synchronize()
    S = O.steps_of(c)
    assert 1 <= steps[0] <= S - 2 and 1 <= steps[1] <= S - 2 and steps[0] != steps[1], steps
    assert int(ppo_g.step[0]) == int(ppo_e.step[0]) == sum(steps)
    for x, y in zip(list(ppo_g.params()) + ppo_g.exp_avg + ppo_g.exp_avg_sq + stats_g, list(ppo_e.params()) + ppo_e.exp_avg + ppo_e.exp_avg_sq + stats_e):
        assert PH.bits(x.detach().cpu().numpy()) == PH.bits(y.detach().cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------------- driver
@pytest.mark.parametrize("wide", (None, True))
def test_driver_with_the_options_and_a_schedule(wide):
    """a smoke run, not a learning curve: both backends, both options, a linear learning-rate schedule"""
    import gym_xarm_amd
    from gym_xarm_amd.train import ActorCritic, linear_schedule, train
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=256, seed=0)
    model, venv, hist = train(env=env, updates=6, algo="ppo", device_update=True, device_policy=True, device_normalize=True, quiet=True, log_every=2,
                              target_kl=0.01, clip_range_vf=0.2, lr=linear_schedule(3e-4), wide=wide)
    assert len(hist) == 3
    for rec in hist:
        assert all(np.isfinite(v) for v in rec.values()) and 0 <= rec["ppo_steps_applied"] <= 16, rec
    assert hist[-1]["ppo_steps_applied"] == 16                                             # the last update runs at lr 0: nothing moves, nothing trips
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    torch.manual_seed(0)
    start = ActorCritic(venv.dim, env.act_dim)
    assert max(float((p.detach().cpu() - q.detach()).abs().max()) for p, q in zip(model.parameters(), start.parameters())) > 1e-4
