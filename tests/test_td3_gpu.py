"""The device-resident TD3 update on the MI355X (gym_xarm_amd/device_td3.py DeviceTD3, csrc/xarm_k_td3.hip): everything a step writes
against the host build of the same core bit for bit, the gradients under the rule of tests/td3_host.py against torch float64, the
device-side delay decision through eager and captured calls, the launch count, the act call, the optimiser hand-over and the driver.
The tests print every case's figures in units of Y; DESIGN.md 28 lists them."""
import copy

import numpy as np
import pytest
import torch

import policy_host as PH
import td3_host as TH
from gym_xarm_amd.device_td3 import DeviceTD3, trained

pytestmark = pytest.mark.gpu
A_, REF = TH.SHAPE_A, TH.SHAPE_REF


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_td3(model, B, h, **kw):
    m = copy.deepcopy(model).cuda()
    return m, DeviceTD3(m, B, gamma=h["gamma"], lr=h["lr"], tau=h["tau"], policy_delay=h["policy_delay"], target_policy_noise=h["target_policy_noise"],
                        target_noise_clip=h["target_noise_clip"], action_noise=h["action_noise"], betas=(h["beta1"], h["beta2"]), eps=h["eps"],
                        seed=h["seed"], **kw)


def dev_batch(b):
    return {k: dev(b[k]) for k in ("obs", "next_obs", "action", "reward", "done", "use") if b[k] is not None}


def cpu(x):
    return x.detach().cpu().numpy()


def state_of(td3):
    return [p.detach().clone() for p in td3.params()] + [t.clone() for t in td3.exp_avg + td3.exp_avg_sq] + [td3.step.clone(), td3.stats.clone()]


def check_case(ref, shape, B, what):
    """one case on the device and in the host build: gradients, y, q, dq1/da, the stats and the whole workspace bit for bit; the gradients
    under the rule against float64"""
    h, b, model = ref["h"], ref["b"], ref["model"]
    _, td3 = device_td3(model, B, h)
    assert td3.launches == 7 * shape[3] + 14 == TH.geometry(B, shape)["launches"]
    td3.buffers["workspace"].zero_()
    for ts, arrs in ((td3.exp_avg, ref["m"]), (td3.exp_avg_sq, ref["v"])):        # the case's warm optimiser state
        for t, a in zip(ts, arrs):
            t.copy_(dev(a))
    g = td3.grad(dev_batch(b), dev(b["z_next"]), lr=h["lr"], step=ref["step"])
    g = {k: cpu(v) for k, v in g.items()}
    w, m, v, step = TH.ref_state(ref)
    rc, host = TH.host_update(w, m, v, step, b, h, shape)
    assert rc == td3.launches
    for k in ("y", "q", "dqda", "grad", "stats"):
        assert PH.bits(g[k]) == PH.bits(host[k]), (what, k)
    n = TH.work_floats(B, shape)
    assert PH.bits(cpu(td3.buffers["workspace"])[:n]) == PH.bits(host["work"][:n]), what
    fig = TH.check_step(g, ref, what)
    print("device TD3 %s: Y %.2e, %d rows settled out, error in Y: %s; the host build's bits"
          % (what, ref["Y"], ref["lost"], " ".join("%s %.2f" % kv for kv in fig.items())))
    assert g["stats"][4] == np.float32(ref["r64"]["stats"]["n_use"])
    return g


@pytest.mark.parametrize("case", TH.CASES, ids=TH.case_id)
def test_a_step_equals_the_host_build_and_gradients_pass_the_rule(case):
    shape, B = case
    check_case(TH.reference(shape, B), shape, B, TH.case_id(case))


def test_a_delayed_step_equals_the_host_build():
    check_case(TH.reference(A_, 200, policy_delay=2, n_updates=1), A_, 200, "delayed")


def test_every_row_range_and_a_one_row_remainder():
    """4 097 rows: 65 tiles dealt to 16 ranges, the last holding the one-row tile; lr = 0 so that the stepped q1 is the call's own"""
    geo = TH.geometry(4097, REF)
    assert geo["S"] == 16 and geo["rows"][0] == 0 and geo["rows"][-1] == 4097 and all(b > a for a, b in zip(geo["rows"], geo["rows"][1:]))
    check_case(TH.reference(REF, 4097, lr=0.0), REF, 4097, "every range, B 4097, lr 0")


@pytest.mark.parametrize("shape", (REF, A_), ids=("256x3", "128x2"))
def test_four_updates_with_policy_delay_2_equal_the_host_build(shape):
    """four real `update` calls: parameters, all targets, Adam's state, `step` and per-call `stats` against the host build bit for bit;
    after calls 1 and 3 the actor and every target hold their bits of before the call, after calls 2 and 4 they do not"""
    B = 200
    h = TH.hyper(policy_delay=2)
    model = TH.make_model(shape)
    batches = [TH.make_batch(shape[0], shape[1], B, seed=s) for s in range(4)]
    _, td3 = device_td3(model, B, h)
    w, m, v, step = TH.fresh_state(model)
    stats = np.zeros(8, np.float32)
    tp = len(w) // 6
    for i, b in enumerate(batches):
        before = [p.detach().clone() for p in td3.params()]
        td3.update(dev_batch(b), dev(b["z_next"]) if i else None)        # the first step draws its own noise
        rc, host = TH.host_update(w, m, v, step, b, h, shape, noise=bool(i), stats=stats)
        assert rc == td3.launches and PH.bits(cpu(td3.stats)) == PH.bits(stats), i
        same = [torch.equal(a, p) for a, p in zip(before, td3.params())]
        quiet = same[:tp] + same[3 * tp:]
        assert all(quiet) if i % 2 == 0 else not any(quiet), i
        assert not any(same[tp:3 * tp]) and float(td3.stats[5]) == float(i % 2)
    assert int(td3.step[0]) == int(step[0]) == 4
    for t, a in zip(td3.params(), w):
        assert PH.bits(cpu(t)) == PH.bits(a)
    for ts, arrs in ((td3.exp_avg, m), (td3.exp_avg_sq, v)):
        for t, a in zip(ts, arrs):
            assert PH.bits(cpu(t)) == PH.bits(a)


@pytest.mark.parametrize("shape", (A_, REF), ids=("L2", "L3"))
def test_launch_count(shape):
    """the kernels one `update` enqueues, counted with the torch profiler: DeviceTD3.launches = 7 n_hidden + 14 on a delayed and on an
    undelayed call alike"""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    B = 65
    b = dev_batch(TH.make_batch(shape[0], shape[1], B))
    _, td3 = device_td3(TH.make_model(shape), B, TH.hyper(policy_delay=2))
    td3.update(b)
    td3.update(b)
    torch.cuda.synchronize()
    for k in range(2):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            td3.update(b)
            torch.cuda.synchronize()
        n = sum(e.count for e in prof.key_averages() if e.device_type == DeviceType.CUDA)
        assert n == td3.launches == 7 * shape[3] + 14, (k, n)
    assert int(td3.step[0]) == 4


def test_two_copies_are_bit_identical():
    shape, B = REF, 200
    batches = [dev_batch(TH.make_batch(shape[0], shape[1], B, seed=s)) for s in range(3)]
    model, h, runs = TH.make_model(shape), TH.hyper(seed=2, policy_delay=2), []
    for _ in range(2):
        _, td3 = device_td3(model, B, h)
        stats = []
        for b in batches:
            td3.update(b)
            stats.append(td3.stats.clone())
        runs.append(state_of(td3) + stats)
        assert int(td3.step[0]) == 3 and bool(torch.isfinite(td3.stats).all())
    for x, y in zip(*runs):
        assert PH.bits(cpu(x)) == PH.bits(cpu(y))


@pytest.mark.parametrize("E", (1, 31, 33, 65, 200))
def test_act_rows_do_not_depend_on_the_batch(E):
    """in every mode: row 7 of 200 against a batch of one with row_offset 7, the first E rows of 200 against a batch of E, and the host build"""
    shape = REF
    D, A = shape[:2]
    model, h = TH.make_model(shape), TH.hyper(seed=5)
    rows = TH.make_batch(D, A, 200)["obs"]
    _, td3 = device_td3(model, 64, h)
    _, one = device_td3(model, 64, h, row_offset=7)
    w = TH.weights_of(model)
    new = lambda n: torch.empty(n, A, device="cuda")
    for mode in ("deterministic", "gaussian", "uniform"):
        td3.calls.fill_(3); one.calls.fill_(3)
        out200 = td3.act_into(new(200), dev(rows), mode).clone()
        assert int(td3.calls[0]) == (3 if mode == "deterministic" else 4)
        td3.calls.fill_(3)
        outE = td3.act_into(new(E), dev(rows[:E]), mode)
        out1 = one.act_into(new(1), dev(rows[7:8]), mode)
        assert PH.bits(cpu(out200[:E])) == PH.bits(cpu(outE)) and PH.bits(cpu(out200[7:8])) == PH.bits(cpu(out1)), mode
        assert PH.bits(cpu(out200)) == PH.bits(TH.host_act(w, rows, shape, h, mode, np.full(1, 3, np.int64))), mode
        assert bool((out200.abs() <= 1).all())
    # predict leaves `calls` alone; uniform draws differ between calls
    c0 = int(td3.calls[0])
    assert torch.equal(td3.predict(dev(rows)), td3.predict(dev(rows))) and int(td3.calls[0]) == c0
    u1 = td3.act_into(new(200), dev(rows), "uniform").clone()
    u2 = td3.act_into(new(200), dev(rows), "uniform")
    assert not torch.equal(u1, u2) and int(td3.calls[0]) == c0 + 2 and float(u1.min()) >= -1.0 and float(u1.max()) <= 1.0


def test_captured_update_replays_the_delay_decision():
    """update captured in a torch.cuda.graph and replayed four times with the batch rewritten in place, policy_delay 2, against four eager
    calls on a twin: bitwise, the step count included - the graph holds ONE set of launches, the device decides which replays step the actor"""
    shape, B = REF, 300
    batches = [dev_batch(TH.make_batch(shape[0], shape[1], B, seed=s)) for s in range(4)]
    model, h = TH.make_model(shape), TH.hyper(seed=3, policy_delay=2)
    _, td3_g = device_td3(model, B, h)
    _, td3_e = device_td3(model, B, h)
    hold = {k: v.clone() for k, v in batches[0].items()}
    td3_g.grad(hold)                              # the kernels are loaded before the capture; the module is not touched
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        td3_g.update(hold)
    stats_g, stats_e, actor = [], [], []
    for b in batches:
        for k in hold:
            hold[k].copy_(b[k])
        graph.replay()
        stats_g.append(td3_g.stats.clone())
        actor.append(td3_g.params()[0].detach().clone())
        td3_e.update(b)
        stats_e.append(td3_e.stats.clone())
    torch.cuda.synchronize()
    assert int(td3_g.step[0]) == int(td3_e.step[0]) == 4
    for x, y in zip(state_of(td3_g) + stats_g, state_of(td3_e) + stats_e):
        assert PH.bits(cpu(x)) == PH.bits(cpu(y))
    start = model.actor[0].weight.detach().cuda()
    assert torch.equal(actor[0], start) and not torch.equal(actor[1], actor[0]) and torch.equal(actor[2], actor[1]) and not torch.equal(actor[3], actor[2])
    assert [float(s[5]) for s in stats_g] == [0.0, 1.0, 0.0, 1.0]


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
        model = TH.make_model((venv.dim, env.action_dim, 256, 3, "relu"))
        sides.append((env, buf, venv) + device_td3(model, B, TH.hyper(seed=1, policy_delay=2)))
    (env_g, buf_g, venv_g, _, td3_g), (env_e, buf_e, venv_e, _, td3_e) = sides
    assert torch.equal(buf_g.ring, buf_e.ring) and torch.equal(venv_g.stats, venv_e.stats)
    n = len(td3_g.params())
    keep = [t.clone() for t in state_of(td3_g)[:n]], buf_g.clock.clone()
    td3_g.update_from(buf_g, venv_g)              # a warm-up call: the graph side is restored after it
    with torch.no_grad():
        for p, q in zip(td3_g.params(), keep[0]):
            p.copy_(q)
    for t in td3_g.exp_avg + td3_g.exp_avg_sq:
        t.zero_()
    td3_g.step.zero_()
    td3_g.stats.zero_()
    buf_g.clock.copy_(keep[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        td3_g.update_from(buf_g, venv_g)
    for k in range(3):
        graph.replay()
        td3_e.update_from(buf_e, venv_e)
    torch.cuda.synchronize()
    assert int(td3_g.step[0]) == 3 == int(td3_e.step[0]) and torch.equal(buf_g.clock, buf_e.clock)
    for x, y in zip(state_of(td3_g), state_of(td3_e)):
        assert PH.bits(cpu(x)) == PH.bits(cpu(y))
    assert float(td3_g.stats[4]) == B and bool(torch.isfinite(td3_g.stats).all())
    env_g.close(); env_e.close()


def test_optimiser_hand_over_in_both_directions():
    """two torch steps on the GPU, DeviceTD3.load_optimizer, a device step; export_optimizer, a torch step: counts and continuity"""
    from gym_xarm_amd.td3 import make_optimizers, td3_step
    shape, B = TH.SHAPE_64, 65
    h = TH.hyper(policy_delay=2)
    model = copy.deepcopy(TH.make_model(shape)).cuda()
    opts = make_optimizers(model, h["lr"])
    batches = [dev_batch(TH.make_batch(shape[0], shape[1], B, seed=s)) for s in range(4)]
    for n in (1, 2):
        td3_step(model, opts, batches[n - 1], n, policy_delay=2)
    td3 = DeviceTD3(model, B, policy_delay=2)
    td3.load_optimizer(opts)
    assert int(td3.step[0]) == 2 and any(bool(t.any()) for t in td3.exp_avg[:6]) and torch.equal(td3.exp_avg[6], opts["critic"].state[model.q1[0].weight]["exp_avg"])
    td3.update(batches[2])
    assert int(td3.step[0]) == 3 and float(td3.stats[5]) == 0.0
    td3.export_optimizer(opts)
    ps = trained(td3.params())
    assert int(opts["actor"].state[ps[0]]["step"]) == 3 // 2 and int(opts["critic"].state[ps[6]]["step"]) == 3
    st = td3_step(model, opts, batches[3], 4, policy_delay=2)
    assert float(st["actor_stepped"]) == 1.0 and int(opts["actor"].state[ps[0]]["step"]) == 2 and all(bool(torch.isfinite(p).all()) for p in model.parameters())
    opts["critic"].state[ps[6]]["step"].fill_(7.0)
    with pytest.raises(ValueError):
        td3.load_optimizer(opts)


@pytest.mark.parametrize("device_normalize", (False, True))
def test_driver_with_the_device_update(device_normalize):
    """a smoke run, not a learning curve"""
    import gym_xarm_amd
    from gym_xarm_amd.td3 import train_td3
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=256, seed=0, config={"reward_type": "sparse", "GUI": False})
    model, venv, hist = train_td3(env=env, steps=80, batch_size=256, device_update=True, device_normalize=device_normalize, quiet=True, log_every=40,
                                  net_arch=(256, 256, 256), activation="relu")
    assert model.net_arch == (256, 256, 256) and model.activation == "relu"
    assert len(hist) == 2 and hist[-1]["updates"] == 30 and hist[-1]["env_steps"] == 80 * 256
    for rec in hist:
        assert all(np.isfinite(v) for v in rec.values()), rec
    assert hist[-1]["n_use"] == 256.0 and hist[-1]["actor_stepped"] == 1.0
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    assert not torch.equal(model.actor_target[0].weight, model.actor[0].weight)


LEARN = dict(num_envs=256, steps=9000, batch_size=256, log_every=1000, net_arch=(256, 256, 256), activation="relu")
# the torch block (train_td3 without the device flags) on this shape, measured on an MI355X (tools/td3_rate.py --learn, 12 000 steps, windows
# of 1 000): success_rate 0.192, 0.721, 0.728, 0.758, 0.769, 0.783, 0.791, 0.797, 0.820, ... - the ninth window is the first above 0.8, so the
# budget is 9 000 steps (44 s for the 12 000); the device path in the same job 0.000, 0.402, 0.854, ..., 0.921 at 9 000 (12 s for the 12 000)
TORCH_GAIN = 0.820 - 0.192


def test_device_td3_learns_sparse_reach_with_her():
    """sparse Reach with HER, 256 envs x 9 000 steps, one TD3 step of 256 rows per env step, [256, 256, 256] ReLU (DESIGN.md 28 records both
    runs).  The pass condition is the gain in success_rate of the last log window over the first: at least half of what the torch block
    gained on the same budget (0.314).  Only the device path runs here: the torch block takes four times as long."""
    from gym_xarm_amd.td3 import train_td3
    model, venv, hist = train_td3("XarmReach-v0", config={"reward_type": "sparse", "GUI": False}, quiet=True, device_update=True, device_normalize=True, **LEARN)
    first, last = hist[0]["success_rate"], hist[-1]["success_rate"]
    print("device TD3 + HER, sparse Reach 256 envs x 9000 steps: success_rate %.4f -> %.4f" % (first, last))
    assert all(np.isfinite(v) for rec in hist for v in rec.values())
    assert last - first >= 0.5 * TORCH_GAIN
