"""The device-resident SAC update on the MI355X (gym_xarm_amd/device_sac.py DeviceSAC, csrc/xarm_k_sac.hip): the per-row quantities
against the host build of the same core bit for bit, the three gradients under the rule of tests/sac_host.py against torch float64 and
against the host build, the tile walk of a workgroup with two tiles, whole steps (repeatable, under the parameter rule), the act call,
captured updates against eager ones, the driver and a learning run on sparse Reach with HER.

Largest error in units of Y over these cases (Y: what torch's float32 autograd loses on the case; tests/sac_host.py): the tests print
every case's figure and DESIGN.md 23 lists them."""
import copy

import numpy as np
import pytest
import torch

import policy_host as PH
import sac_host as SH
from gym_xarm_amd.device_sac import DeviceSAC, trained

pytestmark = pytest.mark.gpu


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


def check_case(r, D, A, B, what):
    """one case on the device and in the host build: y and dq/da bit for bit, the gradients under the rule against float64 and, with
    the same bounds, against the host build"""
    h, b = r["h"], r["b"]
    _, sac = device_sac(r["model"], B, h)
    g = sac.grad(dev_batch(b), dev(b["z_pi"]), dev(b["z_next"]), lr=h["lr"])
    w, m, v, step = SH.fresh_state(r["model"])
    rc, host = SH.host_update(w, m, v, step, b, h)
    assert rc == 0
    assert PH.bits(cpu(g["y"])) == PH.bits(host["y"]) and PH.bits(cpu(g["dqda"])) == PH.bits(host["dqda"]), what
    gd, g64 = cpu(g["grad"]), r["r64"]["grad"]
    res = SH.rule(gd, g64, r["Y"], D, A)
    bd = SH.bounds(g64, r["Y"], D, A)
    # a zero bound (log_alpha's gradient under a fixed coefficient) asks for equality
    vs_host = max((np.abs(a.astype(np.float64) - c).max() / k) if k > 0 else (0.0 if np.array_equal(a, c) else np.inf)
                  for a, c, k in zip(SH.split(gd, D, A), SH.split(host["grad"], D, A), bd))
    by, bq = SH.block_rule(cpu(g["y"]), r["r32"]["y"], r["r64"]["y"]), SH.block_rule(cpu(g["dqda"]), r["r32"]["dqda"], r["r64"]["dqda"])
    print("device SAC %s: Y %.2e, error in Y: actor %.2f critic %.2f log_alpha %.2f, y %.2f, dq/da %.2f; against the host build %.3f of the bound"
          % (what, r["Y"], res["actor"][1], res["critic"][1], res["log_alpha"][1], by[1], bq[1], vs_host))
    for k, (ratio, _) in res.items():
        assert ratio <= 1.0, (what, k, ratio)
    assert vs_host <= 1.0 and by[0] <= 1.0 and bq[0] <= 1.0, (what, vs_host, by, bq)
    st = cpu(g["stats"])
    assert np.isfinite(st).all() and st[6] == np.float32(r["r64"]["stats"]["n_use"]) and st[7] == 0.0
    return max(v[1] for v in res.values())


@pytest.mark.parametrize("scale", (1.0, 4.0))
@pytest.mark.parametrize("D,A", SH.WIDTHS)
def test_rows_equal_the_host_build_and_gradients_pass_the_rule(D, A, scale):
    worst = 0.0
    for B in SH.ROWS:
        worst = max(worst, check_case(SH.reference(D, A, B, scale), D, A, B, "D %d A %d B %d weights x %g" % (D, A, B, scale)))
    print("device SAC gradient D %d A %d weights x %g: largest error %.2f Y" % (D, A, scale, worst))


def test_a_workgroup_walks_a_second_tile():
    """16 385 rows: 257 tiles over 256 workgroups, so workgroup 0 walks a second tile that holds one row"""
    D, A, B = 14, 4, 16385
    assert SH.geometry(B, D, A)[:4] == [257, 256, 64, 256]
    check_case(SH.reference(D, A, B, 1.0), D, A, B, "D %d A %d B %d" % (D, A, B))


def test_fixed_entropy_coefficient_and_the_clamp_case():
    D, A, B = 14, 4, 65
    check_case(SH.reference(D, A, B, 1.0, ent_coef=0.2), D, A, B, "fixed ent_coef")
    r = SH.reference(D, A, B, 1.0, shift=True)
    check_case(r, D, A, B, "log_std clamped on every used row")
    _, sac = device_sac(r["model"], B, r["h"])
    g = SH.split(cpu(sac.grad(dev_batch(r["b"]), dev(r["b"]["z_pi"]), dev(r["b"]["z_next"]), lr=r["h"]["lr"])["grad"]), D, A)
    # every used row sits beyond the upper clamp: the log_std rows of the last layer get exactly nothing, the mean rows do
    assert np.all(g[4].reshape(2 * A, 64)[A:] == 0.0) and np.all(g[5][A:] == 0.0)
    assert np.abs(g[4].reshape(2 * A, 64)[:A]).max() > 0.0 and np.abs(g[5][:A]).max() > 0.0


def test_all_masked_batch_on_the_device():
    """every gradient is exactly zero and `step` advances.  From zero state Adam's step on a zero gradient is p - x (0 / eps) = p: the
    trained tensors keep their bits, Adam's state stays zero, and only the targets move (their Polyak step)"""
    D, A, B = 30, 4, 200
    b = SH.make_batch(D, A, B, 1.0)
    b["use"][:] = 0.0
    model = SH.make_model(D, A)
    _, sac = device_sac(model, B, SH.hyper())
    sac.step.fill_(7)
    g = sac.grad(dev_batch(b), dev(b["z_pi"]), dev(b["z_next"]), lr=1e-3)
    assert bool((g["grad"] == 0).all()) and float(g["stats"][6]) == 1.0 and int(sac.step[0]) == 7
    before = [p.detach().clone() for p in sac.params()]
    sac.update(dev_batch(b), dev(b["z_pi"]), dev(b["z_next"]))
    assert int(sac.step[0]) == 8
    for i, (p, p0) in enumerate(zip(sac.params(), before)):
        if i < 18 or i == 30:
            assert torch.equal(p, p0), i
        else:
            c = before[i - 12]
            assert torch.equal(p, p0 * float(np.float32(1.0 - 0.005)) + c * float(np.float32(0.005))) and not torch.equal(p, p0), i
    assert all(bool((t == 0).all()) for t in sac.exp_avg + sac.exp_avg_sq)


@pytest.mark.parametrize("D,A,B", ((14, 4, 65), (30, 4, 200)))
def test_three_steps_are_repeatable_and_obey_the_parameter_rule(D, A, B):
    runs = []

    def run(model, batches, h):
        _, sac = device_sac(model, B, h)
        for b in batches:
            sac.update(dev_batch(b), dev(b["z_pi"]), dev(b["z_next"]))
        runs.append(state_of(sac))
        assert int(sac.step[0]) == len(batches) and bool(torch.isfinite(sac.stats).all())
        ps = sac.params()
        return np.concatenate([cpu(p).astype(np.float64).ravel() for p in trained(ps)]), np.concatenate([cpu(p).astype(np.float64).ravel() for p in ps[18:30]])
    res, Y, left, worst_t = SH.parameter_case(D, A, B, 3, run)
    print("device SAC parameters D %d A %d B %d after 3 steps: Y %.2e, error in Y: actor %.2f critic %.2f log_alpha %.2f, targets %.3f of the bound, left out %d"
          % (D, A, B, Y, res["actor"][1], res["critic"][1], res["log_alpha"][1], worst_t, left))
    assert all(v[0] <= 1.0 for v in res.values()) and worst_t <= 1.0
    SH.parameter_case(D, A, B, 3, run)
    for x, y in zip(*runs):
        assert PH.bits(cpu(x)) == PH.bits(cpu(y))


def test_act_rows_do_not_depend_on_the_batch_and_equal_the_host_build():
    D, A = 30, 4
    model = SH.make_model(D, A)
    h = SH.hyper(seed=5)
    m, sac = device_sac(model, 64, h, row_offset=100)
    rows = SH.make_batch(D, A, 200, 1.0)["obs"]
    out200 = sac.act_into({"action": torch.empty(200, A, device="cuda"), "logp": torch.empty(200, device="cuda")}, dev(rows))
    assert int(sac.calls[0]) == 1
    sac.calls.zero_()
    out64 = sac.act_into({"action": torch.empty(64, A, device="cuda"), "logp": torch.empty(64, device="cuda")}, dev(rows[:64]))
    for k in ("action", "logp"):
        assert PH.bits(cpu(out200[k][:64])) == PH.bits(cpu(out64[k]))
    w = SH.weights_of(model)
    host = SH.host_act(w, rows, A, h, row_offset=100)
    det = SH.host_act(w, rows, A, h, deterministic=True)
    assert PH.bits(cpu(out200["action"])) == PH.bits(host["action"]) and PH.bits(cpu(out200["logp"])) == PH.bits(host["logp"])
    assert PH.bits(cpu(sac.predict(dev(rows)))) == PH.bits(det["action"]) and int(sac.calls[0]) == 1
    # replays of a captured graph draw fresh noise and advance calls
    o = {"action": torch.empty(200, A, device="cuda")}
    x = dev(rows)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sac.act_into(o, x)
    seen = []
    c0 = int(sac.calls[0])
    for k in range(3):
        graph.replay()
        seen.append(o["action"].clone())
    torch.cuda.synchronize()
    assert int(sac.calls[0]) == c0 + 3
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    calls = np.array([c0 + 2], np.int64)
    assert PH.bits(cpu(seen[2])) == PH.bits(SH.host_act(w, rows, A, h, calls=calls, row_offset=100)["action"]) and calls[0] == c0 + 3


def test_captured_update_replays_as_eager_steps():
    """update captured in a torch.cuda.graph and replayed three times with the batch rewritten in place, against three eager steps on a
    twin (Philox noise from the device step counter): bitwise, the step count included"""
    D, A, B = 30, 4, 300
    batches = [dev_batch(SH.make_batch(D, A, B, 1.0, seed=s)) for s in range(3)]
    model, h = SH.make_model(D, A), SH.hyper(seed=3)
    _, sac_g = device_sac(model, B, h)
    _, sac_e = device_sac(model, B, h)
    assert sac_g.launches == 6 == SH.geometry(B, D, A)[6]
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
    """update_from on a DeviceHerReplayBuffer filled by a 64-env Reach: sample, reward, both normaliser calls and the six launches in one
    graph, replayed three times, against three eager calls on a twin buffer and model"""
    B = 256
    sides = []
    for _ in range(2):
        env, buf, venv = filled_reach()
        model = SH.make_model(venv.dim, env.action_dim)
        sides.append((env, buf, venv) + device_sac(model, B, SH.hyper(seed=1)))
    (env_g, buf_g, venv_g, _, sac_g), (env_e, buf_e, venv_e, _, sac_e) = sides
    assert torch.equal(buf_g.ring, buf_e.ring) and torch.equal(venv_g.stats, venv_e.stats)
    # a warm-up call on a scratch twin state: the graph side is restored after it
    keep = [t.clone() for t in state_of(sac_g)[:31]], buf_g.clock.clone()
    sac_g.update_from(buf_g, venv_g)
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
def test_driver_with_the_device_update(device_normalize):
    """a smoke run, not a learning curve"""
    import gym_xarm_amd
    from gym_xarm_amd.sac import train_sac
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=256, seed=0, config={"reward_type": "sparse", "GUI": False})
    model, venv, hist = train_sac(env=env, steps=80, batch_size=256, device_update=True, device_normalize=device_normalize, quiet=True, log_every=40)
    assert len(hist) == 2 and hist[-1]["updates"] == 30 and hist[-1]["env_steps"] == 80 * 256
    for rec in hist:
        assert all(np.isfinite(v) for v in rec.values()), rec
    assert hist[-1]["n_use"] == 256.0 and venv.monitor.n == 256 * (80 // 25)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


LEARN = dict(num_envs=256, steps=12000, batch_size=256, log_every=1000)
# the torch block (train_sac without the device flags) on this budget, measured on an MI355X: success_rate of the first 1 000-step window
# 0.0035, of the last 0.7147 (52 s); the device path in the same job 0.0037 -> 0.7400 (11.5 s)
TORCH_GAIN = 0.7147 - 0.0035


def test_device_sac_learns_sparse_reach_with_her():
    """sparse Reach with HER, 256 envs x 12 000 steps, one SAC step of 256 rows per env step from step 51 on (DESIGN.md 23 records the
    budget and both runs' figures).  The pass condition is the gain in success_rate of the last log window over the first: at least half
    of what the torch block gained on the same budget (0.3556).  Only the device path runs here: the torch block takes 52 s."""
    from gym_xarm_amd.sac import train_sac
    model, venv, hist = train_sac("XarmReach-v0", config={"reward_type": "sparse", "GUI": False}, quiet=True, device_update=True, device_normalize=True, **LEARN)
    first, last = hist[0]["success_rate"], hist[-1]["success_rate"]
    print("device SAC + HER, sparse Reach 256 envs x 12000 steps: success_rate %.4f -> %.4f" % (first, last))
    assert all(np.isfinite(v) for rec in hist for v in rec.values())
    assert last - first >= 0.5 * TORCH_GAIN
