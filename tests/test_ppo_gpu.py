"""The device-resident PPO update (csrc/xarm_k_ppo.hip) through DevicePPO on the GPU: advantages and returns bit for bit the host
build's, step 0's gradient under the rule of tests/a2c_host.py against float64 autograd and against the host build, the all-masked and
out-of-range-perm calls, run-to-run bits, the parameters after a whole update, the weights a DevicePolicy reads, a captured graph
against eager updates, and train(algo="ppo", device_update=True).

Largest gradient error in units of Y (what torch's float32 autograd loses against float64) is printed per case; DESIGN.md 22 lists the
figures."""
import numpy as np
import pytest
import torch

import a2c_host as AH
import policy_host as PH
import ppo_host as PP

pytestmark = pytest.mark.gpu
ROWS = ((1, 1), (1, 31), (1, 33), (5, 13), (5, 200))     # T x E: one row, under a tile, over the policy kernel's 32-row tile, 65, 1000 rows
BATCHES = (1 << 20, 64, 20)


def device_ppo(D, A, T, E, n_epochs, batch_size, **hyper):
    from gym_xarm_amd.device_ppo import DevicePPO
    model = AH.model_of(D, A, 1.0).cuda()
    h = dict(hyper)
    if "beta1" in h:
        h["betas"] = (h.pop("beta1"), h.pop("beta2"))
    return model, DevicePPO(model, E, n_steps=T, n_epochs=n_epochs, batch_size=min(batch_size, T * E), **h)


def fill(ppo, b, perm):
    """the batch and perm into the updater's buffers, in place; returns last_obs on the device"""
    for k in ("obs", "action", "reward", "done"):
        ppo.buffers[k].copy_(torch.from_numpy(b[k]))
    if b["use"] is None:
        ppo.buffers["use"].fill_(1.0)
    else:
        ppo.buffers["use"].copy_(torch.from_numpy(b["use"]))
    ppo.perm.copy_(torch.from_numpy(perm))
    return torch.from_numpy(b["last_obs"]).cuda()


def dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def within_bounds(x, ref, bounds, D, A):
    """worst |x - ref| / bound over the 13 tensors"""
    return max(np.abs(a - r).max() / bd for a, r, bd in zip(AH.split(np.asarray(x, np.float64), D, A), AH.split(np.asarray(ref, np.float64), D, A), bounds))


def first_step_case(D, A, T, E, B, normalize, ent, supplied):
    r = PP.reference(D, A, T, E, B, normalize, ent, supplied)
    model, ppo = device_ppo(D, A, T, E, 1, B, ent_coef=ent, normalize_advantage=bool(normalize))
    last = fill(ppo, r["b"], r["perm"])
    g, adv, ret, st = ppo.grad(last, dev(r["old_logp"]))
    w, m, v, step = PP.fresh_state(model)
    assert all(PH.bits(w[k]) == PH.bits(PH.case(D, 0, A, 1.0)["w"][k]) for k in PH.NAMES) and int(ppo.step[0]) == 0      # grad() leaves the module alone
    rc, host = PP.host_update(w, m, v, step, r["b"], dict(r["h"], lr=0.0), r["perm"], B, r["old_logp"])
    assert rc == 0
    assert PH.bits(adv.cpu().numpy()) == PH.bits(host["adv"]) and PH.bits(ret.cpu().numpy()) == PH.bits(host["returns"]), (T, E)
    if not supplied:
        # the call-start old_logp is the host build's, bit for bit: every ratio of the first step is exactly 1, and handing the host
        # build's values in gives the same bits in every output
        assert float(st[0, 5]) == 0.0 and float(st[0, 6]) == 0.0
        g2, _, _, st2 = ppo.grad(last, dev(host["old_logp"]))
        assert torch.equal(g, g2) and torch.equal(st, st2)
    g = g.cpu().numpy()
    g64 = r["r64"][0]["grad"]
    ratio, in_y = AH.rule(g, g64, r["Y"], D, A)
    vs_host = within_bounds(g, host["grad"], AH.bounds(g64, r["Y"], D, A), D, A)
    print("device PPO gradient D %d A %d rows %dx%d batch %d norm %d ent %g old_logp %s: Y %.2e, error %.2f Y (%s, %.1e of the model's largest entry), "
          "error / bound %.3f, against the host build / bound %.3f" % ((D, A, T, E, min(B, T * E), normalize, ent, "given" if supplied else "NULL", r["Y"], in_y) +
                                                                      AH.worst_tensor(g, g64, D, A) + (ratio, vs_host)))
    assert ratio <= 1.0 and vs_host <= 1.0, (T, E, B, ratio, vs_host)
    st, hs = st.cpu().numpy(), host["stats"]
    PP.check_stats(st[0], r["r64"][0], r["Y"], A)
    assert st[0][4] == hs[0][4] and st[0][6] == hs[0][6] and st[0][2] == hs[0][2]
    return in_y


@pytest.mark.parametrize("D,A", AH.WIDTHS)
def test_advantages_and_first_step_gradient_against_host_and_float64(D, A):
    worst = 0.0
    for T, E in ROWS:
        for B in BATCHES:
            if B != 1 << 20 and (T * E < 65 or ((D, A) != (14, 4) and T * E > 65)):
                continue
            odd = (T * E + B) % 2
            for normalize, ent, supplied in ((1, 0.01 * odd, True), (1 - odd, 0.0, False)):
                worst = max(worst, first_step_case(D, A, T, E, B, normalize, ent, supplied))
    print("device PPO gradient D %d A %d: largest error %.2f Y" % (D, A, worst))


def test_gradient_when_every_workgroup_loops_and_the_grid_ends_on_a_partial_tile():
    """5 x 16 385 = 81 925 rows in one minibatch: 1 281 tiles of 64 positions over the 256 workgroups per tower - every workgroup walks
    five tiles, workgroup 0 a sixth, which holds the last 5 positions.  Against float64 only."""
    D, A, T, E = 14, 4, 5, 16385
    N = T * E
    tiles, groups, rows, most, B, M, S, launches = PP.geometry(T, E, D, A, 1, N)
    assert groups == most and tiles >= 2 * groups and N % rows != 0 and (tiles - 1) % groups == 0 and (B, M, S, launches) == (N, 1, 1, 7)
    r = PP.reference(D, A, T, E, N, 1, 0.0, True)
    model, ppo = device_ppo(D, A, T, E, 1, N)
    g, adv, ret, st = ppo.grad(fill(ppo, r["b"], r["perm"]), dev(r["old_logp"]))
    ratio, in_y = AH.rule(g.cpu().numpy(), r["r64"][0]["grad"], r["Y"], D, A)
    print("device PPO gradient D %d A %d rows %dx%d: Y %.2e, error %.2f Y, error / bound %.3f" % (D, A, T, E, r["Y"], in_y, ratio))
    assert ratio <= 1.0
    PP.check_stats(st[0].cpu().numpy(), r["r64"][0], r["Y"], A)
    # adv and ret start from float32 values: three dot-product chains of D, 64 and 64 terms, then three roundings per step
    adv64, ret64 = r["prep64"][0].reshape(T, E), r["prep64"][1].reshape(T, E)
    top = max(np.abs(ret64).max(), np.abs(adv64).max())
    assert np.abs(ret.cpu().numpy() - ret64).max() <= (D + 128 + 4 * T) * 2.0 ** -24 * T * top
    assert np.abs(adv.cpu().numpy() - adv64).max() <= (D + 128 + 4 * T) * 2.0 ** -24 * T * top


def test_all_masked_call_on_the_device():
    D, A, T, E, B = 30, 4, 5, 13, 20
    b = PP.make_batch(D, A, T, E, 1.0)
    b["use"][:] = 0.0
    model, ppo = device_ppo(D, A, T, E, 2, B)
    before = [p.detach().clone() for p in ppo.params()]
    ppo.step.fill_(7)
    g = torch.full((ppo.num_params,), float("nan"), device="cuda")
    ppo.update(fill(ppo, b, PP.make_perm(T * E, 2)), shuffle=False, out_grad=g)
    assert bool((g == 0).all()) and int(ppo.step[0]) == 7 + 8 and ppo.stats.shape == (8, 8)
    assert bool((ppo.stats[:, 3] == 0).all()) and bool((ppo.stats[:, 4] == 1).all())
    for p, p0, m, v in zip(ppo.params(), before, ppo.exp_avg, ppo.exp_avg_sq):
        assert torch.equal(p, p0) and bool((m == 0).all()) and bool((v == 0).all())


def test_out_of_range_perm_entries_on_the_device():
    D, A, T, E, B = 14, 4, 5, 13, 20
    b, bad, b0, perm = PP.out_of_range_pair(D, A, T, E)
    olp = dev(PP.spread_old_logp(AH.model_of(D, A, 1.0), b, PP.hyper()))
    res = []
    for batch, pm in ((b, bad), (b0, perm)):
        model, ppo = device_ppo(D, A, T, E, 1, B)
        outs = [torch.full((T, E), float("nan"), device="cuda"), torch.full((T, E), float("nan"), device="cuda"), torch.full((ppo.num_params,), float("nan"), device="cuda")]
        ppo.update(fill(ppo, batch, pm), shuffle=False, old_logp=olp, out_adv=outs[0], out_returns=outs[1], out_grad=outs[2])
        assert int(ppo.step[0]) == 4
        res.append([p.detach().clone() for p in ppo.params()] + ppo.exp_avg + ppo.exp_avg_sq + outs + [ppo.stats])
    for x, y in zip(*res):
        assert bool(torch.isfinite(x).all()) and PH.bits(x.cpu().numpy()) == PH.bits(y.cpu().numpy())
    assert float(res[0][-1][:, 4].sum()) == b0["use"].sum()


@pytest.mark.parametrize("D,A,B", ((14, 4, 20), (30, 4, 1 << 20)))
def test_whole_updates_are_repeatable_and_obey_the_parameter_rule(D, A, B):
    """the same two-epoch update on two copies of a model: bit-identical parameters, Adam state, step and stats; and the parameters
    obey the parameter rule against torch's float64 update, as the host build does (tests/test_ppo_host.py)"""
    T, E = 5, 13
    runs = []

    def run(r):
        model, ppo = device_ppo(D, A, T, E, 2, B)
        ppo.update(fill(ppo, r["b"], r["perm"]), shuffle=False, old_logp=dev(r["old_logp"]))
        runs.append([p.detach().clone() for p in ppo.params()] + ppo.exp_avg + ppo.exp_avg_sq + [ppo.step, ppo.stats])
        assert int(ppo.step[0]) == ppo.num_steps and bool(torch.isfinite(ppo.stats).all()) and bool((ppo.stats[:, 3] > 0).all())
        return np.concatenate([p.detach().cpu().numpy().astype(np.float64).ravel() for p in ppo.params()])
    ratio, in_y, Y, left, S = PP.parameter_case(D, A, T, E, B, 2, run)
    print("device PPO parameters D %d A %d batch %d after %d steps: Y %.2e, error %.2f Y, error / bound %.3f, left out %d" % (D, A, B, S, Y, in_y, ratio, left))
    assert ratio <= 1.0
    run(PP.reference(D, A, T, E, B, 1, 0.0, True, n_epochs=2, n_steps=1 << 20))
    for x, y in zip(*runs):
        assert PH.bits(x.cpu().numpy()) == PH.bits(y.cpu().numpy())


def test_device_policy_sees_the_updated_weights():
    from gym_xarm_amd.device_policy import DevicePolicy
    D, A, T, E = 14, 4, 5, 13
    b = PP.make_batch(D, A, T, E, 1.0)
    model, ppo = device_ppo(D, A, T, E, 2, 20)
    policy = DevicePolicy(model)
    rows = torch.from_numpy(b["obs"][0]).cuda()
    before = policy.act(rows, deterministic=True)
    ppo.update(fill(ppo, b, PP.make_perm(T * E, 2)))             # with its own shuffle
    perm = ppo.perm.cpu().numpy()
    assert all(sorted(perm[ep]) == list(range(T * E)) for ep in range(2)) and not np.array_equal(perm[0], perm[1])
    after = policy.act(rows, deterministic=True)
    host = PH.host_act(PH.weights_of(model), b["obs"][0], D, 0, deterministic=True)       # the policy's host build on the new weights
    for k in ("action", "value"):
        assert PH.bits(after[k].cpu().numpy()) == PH.bits(host[k]) and not torch.equal(after[k], before[k])


def test_captured_update_replays_as_eager_updates():
    """update(shuffle=False) captured in a torch.cuda.graph and replayed three times with the buffers and perm rewritten in place,
    against three eager updates on a twin: bitwise, the step count included"""
    D, A, T, E, B = 30, 4, 5, 200, 300
    N = T * E
    batches = [PP.make_batch(D, A, T, E, 1.0, seed=s) for s in range(3)]
    perms = [PP.make_perm(N, 2, seed=s) for s in range(3)]
    model_g, ppo_g = device_ppo(D, A, T, E, 2, B)
    model_e, ppo_e = device_ppo(D, A, T, E, 2, B)
    assert ppo_g.num_steps == 8 and ppo_g.launches == 28
    last = torch.zeros(E, D, device="cuda")
    fill(ppo_g, batches[0], perms[0])
    ppo_g.grad(last)                             # the kernels are loaded before the capture; the module is not touched
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ppo_g.update(last, shuffle=False)
    stats_g, stats_e = [], []
    for b, pm in zip(batches, perms):
        last.copy_(fill(ppo_g, b, pm))
        graph.replay()
        stats_g.append(ppo_g.stats.clone())
        ppo_e.update(fill(ppo_e, b, pm), shuffle=False)
        stats_e.append(ppo_e.stats.clone())
    torch.cuda.synchronize()
    assert int(ppo_g.step[0]) == int(ppo_e.step[0]) == 24
    for x, y in zip(list(ppo_g.params()) + ppo_g.exp_avg + ppo_g.exp_avg_sq + stats_g, list(ppo_e.params()) + ppo_e.exp_avg + ppo_e.exp_avg_sq + stats_e):
        assert PH.bits(x.detach().cpu().numpy()) == PH.bits(y.detach().cpu().numpy())
    assert not torch.equal(ppo_g.params()[0].detach().cpu(), PH.case(D, 0, A, 1.0)["model"].pi[0].weight.detach())


@pytest.mark.parametrize("device_policy", (False, True))
@pytest.mark.parametrize("device_normalize", (False, True))
def test_driver_with_the_device_update(device_policy, device_normalize):
    """a smoke run, not a learning curve"""
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=256, seed=0)
    model, venv, hist = train(env=env, updates=6, algo="ppo", device_update=True, device_policy=device_policy, device_normalize=device_normalize,
                              quiet=True, log_every=3)
    assert len(hist) == 2
    for rec in hist:
        assert all(np.isfinite(v) for v in rec.values()), rec
    assert hist[-1]["env_steps"] == 6 * 16 * 256 and venv.monitor.n == 256 * (6 * 16 // 25)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_driver_with_the_device_update_under_lazy_auto_reset():
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmPDPickAndPlace-v0", num_envs=256, seed=0, auto_reset="lazy")
    model, venv, hist = train(env=env, updates=7, algo="ppo", device_update=True, device_policy=True, device_normalize=True, quiet=True, log_every=7,
                              auto_reset="lazy")
    assert len(hist) == 1 and all(np.isfinite(v) for v in hist[0].values()), hist
    assert venv.monitor.n >= 256                 # 112 calls: every env has finished its first 50-step episode
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_device_ppo_learns_reach():
    """tests/test_reach.py::test_gpu_a2c_learns_reach's budget (3.08e6 env steps: 94 updates of 16 x 2 048) and threshold with the three
    device flags on.  Measured: the torch PPO block with the same settings -0.1443 -> -0.0784, this run -0.1439 -> -0.0781."""
    from gym_xarm_amd.train import train
    model, venv, hist = train("XarmReach-v0", num_envs=2048, updates=94, algo="ppo", n_steps=16, config={"reward_type": "dense", "GUI": False},
                              log_every=47, quiet=True, device_update=True, device_policy=True, device_normalize=True)
    first, last = hist[0]["mean_raw_reward"], hist[-1]["mean_raw_reward"]
    print("device PPO, Reach 2048 envs x 94 updates: mean_raw_reward %.4f -> %.4f" % (first, last))
    assert last > first + 0.03, (first, last, hist)
