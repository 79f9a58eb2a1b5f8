"""The device-resident A2C update (csrc/xarm_k_a2c.hip) through DeviceA2C on the GPU: returns bit for bit the host build's, the gradient
under the rule of tests/a2c_host.py against float64 autograd and against the host build, run-to-run bits, the parameters a
DevicePolicy reads, a captured graph against eager updates, and train(device_update=True).

Largest gradient error in units of Y (what torch's float32 autograd loses against float64) is printed per case; DESIGN.md 21 lists
the figures."""
import numpy as np
import pytest
import torch

import a2c_host as AH
import policy_host as PH

pytestmark = pytest.mark.gpu
ROWS = ((1, 1), (1, 31), (1, 32), (1, 33), (5, 13), (5, 200))     # T x E: around the policy kernel's 32-row tile and this kernel's 64


def device_a2c(D, A, T, E, scale, **hyper):
    from gym_xarm_amd.device_a2c import DeviceA2C
    model = AH.model_of(D, A, scale).cuda()
    return model, DeviceA2C(model, E, n_steps=T, **hyper)


def fill(a2c, b):
    """the batch into the updater's buffers, in place; returns last_obs on the device"""
    for k in ("obs", "action", "reward", "done"):
        a2c.buffers[k].copy_(torch.from_numpy(b[k]))
    if b["use"] is None:
        a2c.buffers["use"].fill_(1.0)
    else:
        a2c.buffers["use"].copy_(torch.from_numpy(b["use"]))
    return torch.from_numpy(b["last_obs"]).cuda()


def within_bounds(x, ref, bounds, D, A):
    """worst |x - ref| / bound over the 13 tensors"""
    return max(np.abs(a - r).max() / bd for a, r, bd in zip(AH.split(np.asarray(x, np.float64), D, A), AH.split(np.asarray(ref, np.float64), D, A), bounds))


@pytest.mark.parametrize("scale", (1.0, 4.0))
@pytest.mark.parametrize("D,A", AH.WIDTHS)
def test_returns_and_gradient_against_host_and_float64(D, A, scale):
    worst = 0.0
    for T, E in ROWS:
        ent = 0.01 if (T * E) % 2 else 0.0
        r = AH.reference(D, A, T, E, scale, ent)
        model, a2c = device_a2c(D, A, T, E, scale, ent_coef=ent)
        last = fill(a2c, r["b"])
        g, ret, st = a2c.grad(last)
        w = PH.weights_of(model)
        assert all(PH.bits(w[k]) == PH.bits(PH.case(D, 0, A, scale)["w"][k]) for k in PH.NAMES)       # grad() leaves the module alone
        rc, host = AH.host_update(w, AH.zeros_like_weights(w), r["b"], r["h"])
        assert rc == 0
        assert PH.bits(ret.cpu().numpy()) == PH.bits(host["returns"]), (T, E)
        g = g.cpu().numpy()
        ratio, in_y = AH.rule(g, r["g64"], r["Y"], D, A)
        vs_host = within_bounds(g, host["grad"], AH.bounds(r["g64"], r["Y"], D, A), D, A)
        print("device gradient D %d A %d scale %g rows %dx%d: Y %.2e, error %.2f Y (%s, %.1e of the model's largest entry), error / bound %.3f, "
              "against the host build / bound %.3f" % ((D, A, scale, T, E, r["Y"], in_y) + AH.worst_tensor(g, r["g64"], D, A) + (ratio, vs_host)))
        worst = max(worst, in_y)
        assert ratio <= 1.0 and vs_host <= 1.0, (T, E, ratio, vs_host)
        st, hs = st.cpu().numpy().astype(np.float64), host["stats"].astype(np.float64)
        assert st[4] == hs[4] and np.all(st[5:] == 0.0)
        # the losses are float64 sums of the same float32 row terms in another order; the norm follows the gradient
        assert abs(st[0] - hs[0]) <= 2.0 ** -22 * r["st64"]["policy_abs"] and abs(st[1] - hs[1]) <= 2.0 ** -22 * hs[1] and st[2] == hs[2]
        assert abs(st[3] - r["st64"]["grad_norm"]) <= (4.0 * r["Y"] + 2.0 ** -22) * r["st64"]["grad_norm"]
    print("device gradient D %d A %d scale %g: largest error %.2f Y" % (D, A, scale, worst))


def test_gradient_when_every_workgroup_loops_and_the_grid_ends_on_a_partial_tile():
    """5 x 16 385 = 81 925 rows: 1 281 tiles of 64 rows over the 256 workgroups per tower - every workgroup walks five tiles, workgroup 0
    a sixth, which holds the last 5 rows.  Against float64 only (the host build would take several seconds at this size)."""
    D, A, T, E = 14, 4, 5, 16385
    tiles, groups, rows, most = AH.geometry(T, E, D, A)
    assert groups == most and tiles >= 2 * groups and (T * E) % rows != 0 and (tiles - 1) % groups == 0
    r = AH.reference(D, A, T, E, 1.0, 0.0)
    model, a2c = device_a2c(D, A, T, E, 1.0)
    g, ret, st = a2c.grad(fill(a2c, r["b"]))
    ratio, in_y = AH.rule(g.cpu().numpy(), r["g64"], r["Y"], D, A)
    print("device gradient D %d A %d rows %dx%d: Y %.2e, error %.2f Y, error / bound %.3f" % (D, A, T, E, r["Y"], in_y, ratio))
    assert ratio <= 1.0
    # the returns start from a float32 value: three dot-product chains of D, 64 and 64 terms, then one rounding per step
    ret64 = r["ret64"]
    assert np.abs(ret.cpu().numpy() - ret64).max() <= (D + 128 + T) * 2.0 ** -24 * np.abs(ret64).max()
    assert float(st[4]) == float(r["b"]["use"].sum())


def test_all_masked_batch_on_the_device():
    D, A, T, E = 30, 4, 5, 13
    b = AH.make_batch(D, A, T, E, 1.0)
    b["use"][:] = 0.0
    model, a2c = device_a2c(D, A, T, E, 1.0)
    for s in a2c.square_avg:
        s.uniform_(0.0, 0.01)
    before, sq0 = [p.detach().clone() for p in a2c.params()], [s.clone() for s in a2c.square_avg]
    g = torch.full((a2c.num_params,), float("nan"), device="cuda")
    a2c.update(fill(a2c, b), out_grad=g)
    assert bool((g == 0).all()) and float(a2c.stats[3]) == 0.0 and float(a2c.stats[4]) == 1.0
    for p, p0, s, s0 in zip(a2c.params(), before, a2c.square_avg, sq0):
        assert torch.equal(p, p0) and torch.equal(s, torch.tensor(0.99, dtype=torch.float32) * s0)


def test_updates_are_repeatable_and_match_the_host_build():
    """the same three updates on two copies of a model: bit-identical parameters, square_avg and stats; and the parameters obey the
    parameter rule against torch's float64 update, as the host build does (tests/test_a2c_host.py)"""
    D, A, T, E = 30, 4, 5, 200
    batches = [AH.make_batch(D, A, T, E, 1.0, seed=s) for s in range(3)]
    runs = []
    for _ in range(2):
        model, a2c = device_a2c(D, A, T, E, 1.0)
        stats = []
        for b in batches:
            a2c.update(fill(a2c, b))
            stats.append(a2c.stats.clone())
        runs.append(([p.detach().clone() for p in a2c.params()], [s.clone() for s in a2c.square_avg], stats))
    for x, y in zip(runs[0][0] + runs[0][1] + runs[0][2], runs[1][0] + runs[1][1] + runs[1][2]):
        assert PH.bits(x.cpu().numpy()) == PH.bits(y.cpu().numpy())
    assert all(bool(torch.isfinite(s).all()) and float(s[3]) > 0 for s in runs[0][2])
    h = AH.hyper()
    cpu = PH.case(D, 0, A, 1.0)["model"]
    left_out = np.zeros(a2c.num_params, bool)
    for i, b in enumerate(batches):
        before, _ = AH.torch_updates(cpu, batches[:i], h, torch.float64)
        g64, _, _ = AH.torch_grad(before, b, h, torch.float64)
        g32, _, _ = AH.torch_grad(before, b, h, torch.float32)
        left_out |= AH.sensitive(g64, AH.yardstick(g32, g64, D, A), D, A)
    for part in AH.split(left_out, D, A):
        assert part.sum() <= 0.01 * part.size
    m64, _ = AH.torch_updates(cpu, batches, h, torch.float64)
    m32, _ = AH.torch_updates(cpu, batches, h, torch.float32)
    p64 = np.concatenate([p.detach().numpy().ravel() for p in PH.model_params(m64)])
    p32 = AH.flat_of(PH.weights_of(m32))
    p = np.concatenate([x.cpu().numpy().astype(np.float64).ravel() for x in runs[0][0]])
    keep = ~left_out
    Y = AH.yardstick(np.where(keep, p32, p64), p64, D, A)
    ratio, in_y = AH.rule(p, p64, Y, D, A, keep)
    print("device parameters D %d A %d after 3 updates: Y %.2e, error %.2f Y, error / bound %.3f, left out %d" % (D, A, Y, in_y, ratio, left_out.sum()))
    assert ratio <= 1.0


def test_device_policy_sees_the_updated_weights():
    from gym_xarm_amd.device_policy import DevicePolicy
    D, A, T, E = 14, 4, 5, 13
    b = AH.make_batch(D, A, T, E, 1.0)
    model, a2c = device_a2c(D, A, T, E, 1.0)
    policy = DevicePolicy(model)
    rows = torch.from_numpy(b["obs"][0]).cuda()
    before = policy.act(rows, deterministic=True)
    a2c.update(fill(a2c, b))
    after = policy.act(rows, deterministic=True)
    host = PH.host_act(PH.weights_of(model), b["obs"][0], D, 0, deterministic=True)       # the policy's host build on the new weights
    for k in ("action", "value"):
        assert PH.bits(after[k].cpu().numpy()) == PH.bits(host[k]) and not torch.equal(after[k], before[k])


def test_captured_update_replays_as_eager_updates():
    """update() captured in a torch.cuda.graph and replayed three times with the buffers rewritten in place, against three eager
    updates on a twin: bitwise"""
    D, A, T, E = 30, 4, 5, 200
    batches = [AH.make_batch(D, A, T, E, 1.0, seed=s) for s in range(3)]
    model_g, a2c_g = device_a2c(D, A, T, E, 1.0)
    model_e, a2c_e = device_a2c(D, A, T, E, 1.0)
    last = torch.zeros(E, D, device="cuda")
    fill(a2c_g, batches[0])
    a2c_g.grad(last)                             # the kernels are loaded before the capture; the module is not touched
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a2c_g.update(last)
    stats_g, stats_e = [], []
    for b in batches:
        last.copy_(fill(a2c_g, b))
        graph.replay()
        stats_g.append(a2c_g.stats.clone())
        a2c_e.update(fill(a2c_e, b))
        stats_e.append(a2c_e.stats.clone())
    torch.cuda.synchronize()
    for x, y in zip(list(a2c_g.params()) + a2c_g.square_avg + stats_g, list(a2c_e.params()) + a2c_e.square_avg + stats_e):
        assert PH.bits(x.detach().cpu().numpy()) == PH.bits(y.detach().cpu().numpy())
    assert not torch.equal(a2c_g.params()[0].detach().cpu(), PH.case(D, 0, A, 1.0)["model"].pi[0].weight.detach())


@pytest.mark.parametrize("device_policy", (False, True))
@pytest.mark.parametrize("device_normalize", (False, True))
def test_driver_with_the_device_update(device_policy, device_normalize):
    """a smoke run, not a learning curve"""
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=256, seed=0)
    model, venv, hist = train(env=env, updates=20, device_update=True, device_policy=device_policy, device_normalize=device_normalize, quiet=True,
                              log_every=10)
    assert len(hist) == 2
    for rec in hist:
        assert all(np.isfinite(v) for v in rec.values()), rec
    assert hist[-1]["env_steps"] == 20 * 5 * 256 and venv.monitor.n == 20 * 5 * 256 // 25
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_driver_with_the_device_update_under_lazy_auto_reset():
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmPDPickAndPlace-v0", num_envs=256, seed=0, auto_reset="lazy")
    model, venv, hist = train(env=env, updates=20, device_update=True, device_policy=True, device_normalize=True, quiet=True, log_every=10,
                              auto_reset="lazy")
    assert len(hist) == 2
    for rec in hist:
        assert all(np.isfinite(v) for v in rec.values()), rec
    assert venv.monitor.n >= 256                 # 100 calls: every env has finished its first 50-step episode
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_device_update_learns_reach():
    """tests/test_reach.py::test_gpu_a2c_learns_reach's run and threshold with the three device flags on"""
    from gym_xarm_amd.train import train
    model, venv, hist = train("XarmReach-v0", num_envs=2048, updates=300, config={"reward_type": "dense", "GUI": False}, log_every=50, quiet=True,
                              device_update=True, device_policy=True, device_normalize=True)
    first, last = hist[0]["mean_raw_reward"], hist[-1]["mean_raw_reward"]
    print("device update, Reach 2048 envs x 300 updates: mean_raw_reward %.4f -> %.4f" % (first, last))
    assert last > first + 0.03, (first, last, hist)
