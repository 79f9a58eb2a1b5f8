"""The wide device-resident SAC update on the MI355X (gym_xarm_amd/device_sac.py DeviceSAC's "wide" backend, csrc/xarm_k_sacw.hip): the
per-row quantities against the host build of the same core bit for bit, the three gradients under the rule of tests/sacw_host.py against
torch float64 and against the host build, the largest row-range count, the 64-64 tanh cross-check against the tile64 backend, whole steps
on two copies, the act call, captured updates against eager ones and the driver.  The tests print every case's figures in units of Y;
DESIGN.md 24 lists them."""
import copy

import numpy as np
import pytest
import torch

import policy_host as PH
import sac_host as SH
import sacw_host as WH
from gym_xarm_amd.device_sac import DeviceSAC, trained

pytestmark = pytest.mark.gpu
REF = WH.SHAPE_REF


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_sac(model, B, h, **kw):
    m = copy.deepcopy(model).cuda()
    return m, DeviceSAC(m, B, gamma=h["gamma"], lr=h["lr"], tau=h["tau"], ent_coef=h["ent_coef"], target_entropy=h["target_entropy"],
                        betas=(h["beta1"], h["beta2"]), eps=h["eps"], seed=h["seed"], **kw)


def dev_batch(b):
    return {k: dev(b[k]) for k in ("obs", "next_obs", "action", "reward", "done", "use") if b[k] is not None}


def cpu(x):
    return x.detach().cpu().numpy()


def state_of(sac):
    return [p.detach().clone() for p in sac.params()] + [t.clone() for t in sac.exp_avg + sac.exp_avg_sq] + [sac.step.clone(), sac.stats.clone()]


def check_case(ref, shape, B, what, start_only=False, **kw):
    """one case on the device and in the host build: a, logp (through the act call and through the update), y, q, dq/da, the gradients
    and the stats bit for bit - the whole workspace is, with a_pi, logp_pi, a', logp' in it; the gradients under the rule against float64"""
    h, b, model = ref["h"], ref["b"], ref["model"]
    A = shape[1]
    _, sac = device_sac(model, B, h, **kw)
    assert sac.backend == "wide" and sac.launches == 6 * shape[3] + 11 == WH.geometry(B, shape)["launches"]
    g = sac.grad(dev_batch(b), dev(b["z_pi"]), dev(b["z_next"]), lr=h["lr"])
    g = {k: cpu(v) for k, v in g.items()}
    w, m, v, step = WH.fresh_state(model)
    rc, host = WH.host_update(w, m, v, step, b, h, shape)
    assert rc == 0
    for k in ("y", "q", "dqda", "grad", "stats"):
        assert PH.bits(g[k]) == PH.bits(host[k]), (what, k)
    # both builds run the same chain over the same workspace: a_pi, logp_pi, a', logp' and z_pi as the update's actor passes left them
    # (and every activation, delta and partial) bit for bit; the rows against float64 as well
    n = WH.work_floats(B, shape)
    work = cpu(sac.buffers["workspace"])[:n]
    assert PH.bits(work) == PH.bits(host["work"][:n]), what
    WH.check_rows(work, ref, B, shape, what)
    # a and logp through the act call; through the update they enter y (a', logp') and dq/da (a_pi), whose bits are compared above
    out = sac.act_into({"action": torch.empty(B, A, device="cuda"), "logp": torch.empty(B, device="cuda")}, dev(b["obs"]))
    ha = WH.host_act(WH.weights_of(model), b["obs"], shape, h)
    assert PH.bits(cpu(out["action"])) == PH.bits(ha["action"]) and PH.bits(cpu(out["logp"])) == PH.bits(ha["logp"]), what
    fig = WH.check_step(g, ref, what, start_only)
    print("device wide SAC %s: Y %.2e, margin %.1e, %d rows settled out, error in Y: %s; the host build's bits"
          % (what, ref["Y"], ref["margin"], ref["lost"], " ".join("%s %.2f" % kv for kv in fig.items())))
    assert g["stats"][6] == np.float32(ref["r64"]["stats"]["n_use"])
    return g


@pytest.mark.parametrize("case", WH.CASES, ids=WH.case_id)
def test_rows_equal_the_host_build_and_gradients_pass_the_rule(case):
    shape, B = case
    check_case(WH.reference(shape, B), shape, B, WH.case_id(case))


def test_the_update_and_the_act_call_give_a_row_the_same_bits():
    """one forward definition: logp of a row through the update's actor pass and through xarm_sacw_act.  The two calls key their Philox
    draws differently, so the comparison runs at z = 0: the update is fed z_pi = 0 and the act call is deterministic - the same u = mean,
    the same terms.  With one used row stats[4], the mean of logp_pi, IS the row's logp_pi (the float64 sum of one float32 over n_use = 1)"""
    shape, B = REF, 1
    ref = WH.reference(shape, B)
    b = dict(ref["b"], z_pi=np.zeros_like(ref["b"]["z_pi"]), use=None)
    _, sac = device_sac(ref["model"], B, ref["h"])
    g = sac.grad(dev_batch(b), dev(b["z_pi"]), dev(b["z_next"]))
    out = sac.act_into({"action": torch.empty(B, shape[1], device="cuda"), "logp": torch.empty(B, device="cuda")}, dev(b["obs"]), deterministic=True)
    assert PH.bits(cpu(g["stats"][4:5])) == PH.bits(cpu(out["logp"]))


def test_every_row_range_and_a_one_row_remainder():
    """B = 64 S + 1 with S the build's largest range count would be 1 025 rows; the case is also not fewer than 4 097: 65 tiles dealt to
    16 ranges of 4 or 5 tiles, the last holding the one-row tile.  Two runs.  With lr = 0 (`grad`'s default; the torch pair runs its Adams
    with lr = 0 too) the critics at the actor step are the critics at call start, so all five evaluations are at the call's own
    parameters, the settle step does not depend on the mask and comes to rest, and EVERY gradient - the actor's through all 16 ranges
    included - y, q, dq/da and the stats are held to float64 under the rule.  With lr = 1e-3 the stepped critics move whenever a row is
    taken out (Adam's first step is lr sign(g)) and the settle step does not come to rest for their two evaluations inside the cap
    (1 287 of 4 097 rows after 12 passes): there the critics' and log_alpha's gradients, y and q are held to float64 and everything -
    the actor's gradient and dq/da too - to the host build's bits."""
    geo = WH.geometry(4097, REF)
    assert geo["max_split"] == 16 and geo["S"] == 16 and geo["split_rows"] == 64 and 64 * geo["max_split"] + 1 <= 4097
    assert geo["rows"][0] == 0 and geo["rows"][-1] == 4097 and all(b > a for a, b in zip(geo["rows"], geo["rows"][1:])) and geo["rows"][-2] % 64 == 0
    check_case(WH.reference(REF, 4097, lr=0.0), REF, 4097, "every range, B 4097, lr 0")
    check_case(WH.reference(REF, 4097, evals="start"), REF, 4097, "every range, B 4097", start_only=True)


def test_wide_backend_on_the_64_64_tanh_shape_against_the_tile():
    """wide=True on a 64-64 tanh model against float64 under the rule, and against the tile64 backend on the same batch: both lie within
    the rule's bound of float64, so within twice the bound of each other (not bitwise: the chains' k orders differ)"""
    shape, B = WH.CROSS
    ref = WH.reference(shape, B)
    g = check_case(ref, shape, B, "wide=True " + WH.case_id(WH.CROSS), wide=True)
    h, b = ref["h"], ref["b"]
    _, tile = device_sac(ref["model"], B, h)
    assert tile.backend == "tile64" and tile.launches == 6
    gt = cpu(tile.grad(dev_batch(b), dev(b["z_pi"]), dev(b["z_next"]), lr=h["lr"])["grad"])
    bd = WH.bounds(ref["r64"]["grad"], ref["Y"], ref["sz"], ref["grp"])
    for a, c, k in zip(WH.split(g["grad"], ref["sz"]), WH.split(gt, ref["sz"]), bd):
        assert np.abs(a.astype(np.float64) - c).max() <= 2.0 * k


def test_fixed_entropy_coefficient():
    shape, B = WH.SHAPE_A, 65
    g = check_case(WH.reference(shape, B, ent_coef=0.2), shape, B, "fixed ent_coef")
    assert g["stats"][3] == np.float32(0.2) and g["stats"][2] == 0.0 and g["grad"][-1] == 0.0


def test_all_masked_batch_on_the_device():
    """every gradient is exactly zero and `step` advances; from zero state the trained tensors keep their bits, Adam's state stays zero,
    and only the targets move (their Polyak step)"""
    shape, B = REF, 200
    D, A = shape[:2]
    b = SH.make_batch(D, A, B, 1.0)
    b["use"][:] = 0.0
    _, sac = device_sac(WH.make_model(shape), B, SH.hyper())
    sac.step.fill_(7)
    g = sac.grad(dev_batch(b), dev(b["z_pi"]), dev(b["z_next"]), lr=1e-3)
    assert bool((g["grad"] == 0).all()) and float(g["stats"][6]) == 1.0 and int(sac.step[0]) == 7
    before = [p.detach().clone() for p in sac.params()]
    sac.update(dev_batch(b), dev(b["z_pi"]), dev(b["z_next"]))
    assert int(sac.step[0]) == 8
    tp = (len(before) - 1) // 5
    for i, (p, p0) in enumerate(zip(sac.params(), before)):
        if i < 3 * tp or i == 5 * tp:
            assert torch.equal(p, p0), i
        else:
            c = before[i - 2 * tp]
            assert torch.equal(p, p0 * float(np.float32(1.0 - 0.005)) + c * float(np.float32(0.005))) and not torch.equal(p, p0), i
    assert all(bool((t == 0).all()) for t in sac.exp_avg + sac.exp_avg_sq)


@pytest.mark.parametrize("shape,B,cap", ((WH.SHAPE_REF, 200, 0.08), (WH.SHAPE_A, 200, 0.01)), ids=("256x3", "128x2"))
def test_three_updates_equal_the_host_build_and_obey_the_parameter_rule(shape, B, cap):
    """three real `update` calls: parameters, targets, Adam's state, `step` and `stats` against three steps of the host build bit for
    bit (apply_param's index mapping, Adam and Polyak on the device), and against torch under DESIGN.md 23's parameter rule on the entries
    the reference keeps (tests/test_sacw_host.py PARAMETER_CASES has the caps and their reasons)"""
    def run(model, batches, h):
        _, sac = device_sac(model, B, h)
        w, m, v, step = WH.fresh_state(model)
        for b in batches:
            sac.update(dev_batch(b), dev(b["z_pi"]), dev(b["z_next"]))
            rc, host = WH.host_update(w, m, v, step, b, h, shape)
            assert rc == 0 and PH.bits(cpu(sac.stats)) == PH.bits(host["stats"])
        assert int(sac.step[0]) == int(step[0]) == len(batches)
        for t, a in zip(sac.params(), w):
            assert PH.bits(cpu(t)) == PH.bits(a)
        for ts, arrs in ((sac.exp_avg, m), (sac.exp_avg_sq, v)):
            for t, a in zip(ts, arrs):
                assert PH.bits(cpu(t)) == PH.bits(a)
        ps = sac.params()
        tp = (len(ps) - 1) // 5
        return np.concatenate([cpu(p).astype(np.float64).ravel() for p in trained(ps)]), np.concatenate([cpu(p).astype(np.float64).ravel() for p in ps[3 * tp:5 * tp]])
    res, Y, share, worst_t = WH.parameter_case(shape, B, 3, run, cap)
    print("device wide SAC parameters %s after 3 steps: Y %.2e, error in Y: %s, targets %.3f of the bound, %.2f %% of a tensor left out"
          % (WH.case_id((shape, B)), Y, " ".join("%s %.2f" % (k, x[1]) for k, x in res.items()), worst_t, 100 * share))
    assert all(x[0] <= 1.0 for x in res.values()) and worst_t <= 1.0


def test_three_steps_on_two_copies_are_bit_identical():
    shape, B = REF, 200
    D, A = shape[:2]
    batches = [SH.make_batch(D, A, B, 1.0, seed=s) for s in range(3)]
    model, h, runs = WH.make_model(shape), SH.hyper(seed=2), []
    for _ in range(2):
        _, sac = device_sac(model, B, h)
        stats = []
        for k, b in enumerate(batches):
            sac.update(dev_batch(b), *((dev(b["z_pi"]), dev(b["z_next"])) if k else ()))     # the first step draws its own noise
            stats.append(sac.stats.clone())
        runs.append(state_of(sac) + stats)
        assert int(sac.step[0]) == 3 and bool(torch.isfinite(sac.stats).all())
    for x, y in zip(*runs):
        assert PH.bits(cpu(x)) == PH.bits(cpu(y))
    assert not torch.equal(runs[0][0].cpu(), model.actor[0].weight.detach())


@pytest.mark.parametrize("E", (1, 31, 33, 65, 200))
def test_act_rows_do_not_depend_on_the_batch(E):
    """row 7 of 200 against a batch of one with row_offset 7, and the first min(E, 200) rows of a batch of E against the batch of 200"""
    shape = REF
    D, A = shape[:2]
    model, h = WH.make_model(shape), SH.hyper(seed=5)
    rows = SH.make_batch(D, A, 200, 1.0)["obs"]
    _, sac = device_sac(model, 64, h)
    new = lambda n: {"action": torch.empty(n, A, device="cuda"), "logp": torch.empty(n, device="cuda")}
    out200 = sac.act_into(new(200), dev(rows))
    sac.calls.zero_()
    outE = sac.act_into(new(E), dev(rows[:E]))
    _, one = device_sac(model, 64, h, row_offset=7)
    out1 = one.act_into(new(1), dev(rows[7:8]))
    for k in ("action", "logp"):
        assert PH.bits(cpu(out200[k][:E])) == PH.bits(cpu(outE[k]))
        assert PH.bits(cpu(out200[k][7:8])) == PH.bits(cpu(out1[k]))


def test_captured_act_draws_fresh_noise():
    shape = REF
    D, A = shape[:2]
    model, h = WH.make_model(shape), SH.hyper(seed=5)
    rows = SH.make_batch(D, A, 200, 1.0)["obs"]
    _, sac = device_sac(model, 64, h, row_offset=100)
    o, x = {"action": torch.empty(200, A, device="cuda")}, dev(rows)
    sac.act_into(o, x)                            # the kernels are loaded and the act workspace exists before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sac.act_into(o, x)
    seen, c0 = [], int(sac.calls[0])
    for k in range(3):
        graph.replay()
        seen.append(o["action"].clone())
    torch.cuda.synchronize()
    assert int(sac.calls[0]) == c0 + 3
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    calls = np.array([c0 + 2], np.int64)
    w = WH.weights_of(model)
    assert PH.bits(cpu(seen[2])) == PH.bits(WH.host_act(w, rows, shape, h, calls=calls, row_offset=100)["action"]) and calls[0] == c0 + 3
    assert PH.bits(cpu(sac.predict(x))) == PH.bits(WH.host_act(w, rows, shape, h, deterministic=True)["action"]) and int(sac.calls[0]) == c0 + 3


def test_captured_update_replays_as_eager_steps():
    """update captured in a torch.cuda.graph and replayed three times with the batch rewritten in place, against three eager steps on a
    twin (Philox noise from the device step counter): bitwise, the step count included"""
    shape, B = REF, 300
    D, A = shape[:2]
    batches = [dev_batch(SH.make_batch(D, A, B, 1.0, seed=s)) for s in range(3)]
    model, h = WH.make_model(shape), SH.hyper(seed=3)
    _, sac_g = device_sac(model, B, h)
    _, sac_e = device_sac(model, B, h)
    hold = {k: v.clone() for k, v in batches[0].items()}
    sac_g.grad(hold)                              # the kernels are loaded before the capture; the module is not touched
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sac_g.update(hold)
    stats_g, stats_e = [], []
    for b in batches:
        for k in hold:
            hold[k].copy_(b[k])
        graph.replay()
        stats_g.append(sac_g.stats.clone())
        sac_e.update(b)
        stats_e.append(sac_e.stats.clone())
    torch.cuda.synchronize()
    assert int(sac_g.step[0]) == int(sac_e.step[0]) == 3
    for x, y in zip(state_of(sac_g) + stats_g, state_of(sac_e) + stats_e):
        assert PH.bits(cpu(x)) == PH.bits(cpu(y))
    assert not torch.equal(sac_g.params()[0].detach().cpu(), model.actor[0].weight.detach())


def filled_reach(E=64, steps=60, seed=0):
    import gym_xarm_amd
    from gym_xarm_amd.her import DeviceHerReplayBuffer, collect
    from gym_xarm_amd.normalize import DeviceVecNormalize
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=E, seed=seed, config={"reward_type": "sparse", "GUI": False})
    buf = DeviceHerReplayBuffer(env, seed=seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    obs = collect(env, buf, lambda o: torch.rand(E, env.action_dim, device="cuda", generator=g) * 2 - 1, steps)
    venv = DeviceVecNormalize(env)
    venv.reset_from(obs)
    return env, buf, venv


def test_captured_update_from_the_replay_buffer():
    """update_from on a DeviceHerReplayBuffer filled by a 64-env Reach: sample, reward, both normaliser calls and the step's launches in
    one graph, replayed three times, against three eager calls on a twin buffer and model"""
    B = 256
    sides = []
    for _ in range(2):
        env, buf, venv = filled_reach()
        model = WH.make_model((venv.dim, env.action_dim, 256, 3, "relu"))
        sides.append((env, buf, venv) + device_sac(model, B, SH.hyper(seed=1)))
    (env_g, buf_g, venv_g, _, sac_g), (env_e, buf_e, venv_e, _, sac_e) = sides
    assert torch.equal(buf_g.ring, buf_e.ring) and torch.equal(venv_g.stats, venv_e.stats)
    n = len(sac_g.params())
    keep = [t.clone() for t in state_of(sac_g)[:n]], buf_g.clock.clone()
    sac_g.update_from(buf_g, venv_g)              # a warm-up call: the graph side is restored after it
    with torch.no_grad():
        for p, q in zip(sac_g.params(), keep[0]):
            p.copy_(q)
    for t in sac_g.exp_avg + sac_g.exp_avg_sq:
        t.zero_()
    sac_g.step.zero_()
    buf_g.clock.copy_(keep[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sac_g.update_from(buf_g, venv_g)
    for k in range(3):
        graph.replay()
        sac_e.update_from(buf_e, venv_e)
    torch.cuda.synchronize()
    assert int(sac_g.step[0]) == 3 == int(sac_e.step[0]) and torch.equal(buf_g.clock, buf_e.clock)
    for x, y in zip(state_of(sac_g), state_of(sac_e)):
        assert PH.bits(cpu(x)) == PH.bits(cpu(y))
    assert float(sac_g.stats[6]) == B and bool(torch.isfinite(sac_g.stats).all())
    env_g.close(); env_e.close()


@pytest.mark.parametrize("device_normalize", (False, True))
def test_driver_with_the_wide_device_update(device_normalize):
    """a smoke run, not a learning curve"""
    import gym_xarm_amd
    from gym_xarm_amd.sac import train_sac
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=256, seed=0, config={"reward_type": "sparse", "GUI": False})
    model, venv, hist = train_sac(env=env, steps=80, batch_size=256, device_update=True, device_normalize=device_normalize, quiet=True, log_every=40,
                                  net_arch=(256, 256, 256), activation="relu")
    assert model.net_arch == (256, 256, 256) and model.activation == "relu"
    assert len(hist) == 2 and hist[-1]["updates"] == 30 and hist[-1]["env_steps"] == 80 * 256
    for rec in hist:
        assert all(np.isfinite(v) for v in rec.values()), rec
    assert hist[-1]["n_use"] == 256.0
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_predict_is_deterministic_on_twin_envs():
    """predict on raw observations of two envs built alike: the same actions, call after call, and `calls` untouched"""
    import gym_xarm_amd
    shape = None
    acts = []
    for _ in range(2):
        env = gym_xarm_amd.make("XarmReach-v0", num_envs=64, seed=3, config={"reward_type": "sparse", "GUI": False})
        obs = env.reset()
        x = torch.cat([obs["observation"], obs["achieved_goal"], obs["desired_goal"]], dim=1).contiguous()
        shape = (x.shape[1], env.action_dim, 256, 3, "relu")
        _, sac = device_sac(WH.make_model(shape), 64, SH.hyper())
        a = sac.predict(x)
        assert torch.equal(a, sac.predict(x)) and int(sac.calls[0]) == 0 and bool((a.abs() <= 1).all())
        acts.append(a.clone())
        env.close()
    assert torch.equal(acts[0], acts[1])


LEARN = dict(num_envs=256, steps=12000, batch_size=256, log_every=1000, net_arch=(256, 256, 256), activation="relu")
# the torch block (train_sac without the device flags) on this budget and shape, measured on an MI355X (tools/sacw_rate.py --learn):
# success_rate of the first 1 000-step window 0.003, of the last 0.991 (60 s); the device path in the same job 0.004 -> 0.976 (13 s)
TORCH_GAIN = 0.991 - 0.003


def test_wide_device_sac_learns_sparse_reach_with_her():
    """sparse Reach with HER, 256 envs x 12 000 steps, one SAC step of 256 rows per env step, [256, 256, 256] ReLU (DESIGN.md 24 records
    both runs).  The pass condition is the gain in success_rate of the last log window over the first: at least half of what the torch
    block gained on the same budget (0.494).  Only the device path runs here: the torch block takes a minute."""
    from gym_xarm_amd.sac import train_sac
    model, venv, hist = train_sac("XarmReach-v0", config={"reward_type": "sparse", "GUI": False}, quiet=True, device_update=True, device_normalize=True, **LEARN)
    first, last = hist[0]["success_rate"], hist[-1]["success_rate"]
    print("wide device SAC + HER, sparse Reach 256 envs x 12000 steps: success_rate %.4f -> %.4f" % (first, last))
    assert all(np.isfinite(v) for rec in hist for v in rec.values())
    assert last - first >= 0.5 * TORCH_GAIN
