"""The wide device-resident PPO update (csrc/xarm_k_ppow.hip) through DevicePPO's "wide" backend on the GPU.  Everything the call writes -
advantages, returns, old_logp, step 0's gradient, the stats, the whole workspace, and parameters / Adam state / step after three real
updates - is held to the host build's BITS (tests/hostbuild_ppow), and the gradient and the stats to the rule of tests/ppow_host.py
against float64 autograd; then the all-masked and out-of-range-perm calls, the cross-check against the "tile64" backend, all 16 row
ranges, a captured update, the driver, and a learning run.  DESIGN.md 25 lists the figures the tests print."""
import json
import os

import numpy as np
import pytest
import torch

import policy_host as PH
import ppo_host as PP
import ppow_host as W

pytestmark = pytest.mark.gpu


def device_ppo(shape, T, E, n_epochs, batch_size, wide=None, **hyper):
    from gym_xarm_amd.device_ppo import DevicePPO
    model = W.model_of(shape).cuda()
    h = dict(hyper)
    if "beta1" in h:
        h["betas"] = (h.pop("beta1"), h.pop("beta2"))
    ppo = DevicePPO(model, E, n_steps=T, n_epochs=n_epochs, batch_size=batch_size, wide=wide, **h)
    return model, ppo


def fill(ppo, b, perm):
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


def same_bits(x, y):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
    y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y
    return x.shape == y.shape and PH.bits(x) == PH.bits(y)


def first_step(shape, T, E, B, normalize, ent, supplied):
    r = W.reference(shape, T, E, B, normalize, ent, supplied)
    model, ppo = device_ppo(shape, T, E, 1, B, wide=True, ent_coef=ent, normalize_advantage=bool(normalize))
    assert ppo.backend == "wide" and ppo.launches == W.geometry(T, E, shape, 1, B)["launches"]
    last = fill(ppo, r["b"], r["perm"])
    g, adv, ret, st = ppo.grad(last, dev(r["old_logp"]))
    w, m, v, step = W.fresh_state(model)
    rc, host = W.host_update(w, m, v, step, r["b"], dict(r["h"], lr=0.0), r["perm"], B, shape, r["old_logp"])
    assert rc == 0
    assert same_bits(adv, host["adv"]) and same_bits(ret, host["returns"]) and same_bits(g, host["grad"]) and same_bits(st, host["stats"])
    assert same_bits(ppo.buffers["workspace"], host["workspace"])                   # old_logp, mean, value, the last step's activations and deltas
    if not supplied:
        assert float(st[0, 5]) == 0.0 and float(st[0, 6]) == 0.0                     # every ratio of step 0 is exactly 1
    ratio, in_y = W.rule(g.cpu().numpy(), r["r64"][0]["grad"], r["Y"], r["sizes"])
    print("wide device PPO gradient %s batch %d norm %d ent %g old_logp %s: Y %.2e, error %.2f Y, error / bound %.3f, settled out %d"
          % (W.case_id((shape, T, E)), B, normalize, ent, "given" if supplied else "NULL", r["Y"], in_y, ratio, r["taken"]))
    assert ratio <= 1.0
    PP.check_stats(st[0].cpu().numpy(), r["r64"][0], r["Y"], shape[1])
    adv64, ret64 = r["prep64"][0].reshape(T, E), r["prep64"][1].reshape(T, E)
    top = max(np.abs(ret64).max(), np.abs(adv64).max())
    bound = (shape[0] + shape[2] * shape[3] + 4 * T) * 2.0 ** -24 * T * top           # DESIGN.md 22's bound with the chains of this shape
    assert np.abs(ret.cpu().numpy() - ret64).max() <= bound and np.abs(adv.cpu().numpy() - adv64).max() <= bound
    return in_y


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_first_step_equals_the_host_build_and_obeys_the_rule(case):
    shape, T, E = case
    for normalize, ent, supplied in ((1, 0.01, True), (1, 0.0, False)):
        first_step(shape, T, E, W.BATCH, normalize, ent, supplied)
    if (T, E) == (5, 13):
        first_step(shape, T, E, W.BATCH, 0, 0.0, True)


def test_wide_backend_on_the_default_shape_against_the_fused_tile():
    """wide=True on a 64-64 tanh model and the "tile64" backend on the same model and batch: both within the rule's bound of float64"""
    shape, T, E, B = W.SHAPE_CROSS, 5, 13, W.BATCH
    r = W.reference(shape, T, E, B, 1, 0.0, True)
    grads = {}
    for wide in (True, None):
        model, ppo = device_ppo(shape, T, E, 1, B, wide=wide)
        grads[ppo.backend] = ppo.grad(fill(ppo, r["b"], r["perm"]), dev(r["old_logp"]))
    assert sorted(grads) == ["tile64", "wide"]
    for k, (g, adv, ret, st) in grads.items():
        ratio, in_y = W.rule(g.cpu().numpy(), r["r64"][0]["grad"], r["Y"], r["sizes"])
        print("backend %s on 64-64 tanh: error %.2f Y, error / bound %.3f" % (k, in_y, ratio))
        assert ratio <= 1.0
        PP.check_stats(st[0].cpu().numpy(), r["r64"][0], r["Y"], shape[1])


def test_all_sixteen_row_ranges_and_a_one_row_tile():
    shape, T, E = W.SHAPE_A, 1, 4097
    N = T * E
    geo = W.geometry(T, E, shape, 1, N)
    assert geo["ranges"] == 16 and geo["rows"][16] == N and (N - geo["rows"][15]) % 64 == 1 and geo["M"] == 1
    r = W.reference(shape, T, E, N, 1, 0.0, True)
    model, ppo = device_ppo(shape, T, E, 1, N, lr=0.0)
    g = torch.full((ppo.num_params,), float("nan"), device="cuda")
    ppo.update(fill(ppo, r["b"], r["perm"]), shuffle=False, old_logp=dev(r["old_logp"]), out_grad=g)
    w, m, v, step = W.fresh_state(model)
    rc, host = W.host_update(w, m, v, step, r["b"], dict(r["h"], lr=0.0), r["perm"], N, shape, r["old_logp"])
    assert rc == 0 and same_bits(g, host["grad"]) and same_bits(ppo.stats, host["stats"])
    ratio, in_y = W.rule(g.cpu().numpy(), r["r64"][0]["grad"], r["Y"], r["sizes"])
    print("wide device PPO gradient %s: Y %.2e, error %.2f Y, error / bound %.3f, settled out %d" % (W.case_id((shape, T, E)), r["Y"], in_y, ratio, r["taken"]))
    assert ratio <= 1.0


@pytest.mark.parametrize("shape", (W.SHAPE_REF, W.SHAPE_ODD), ids=lambda s: "D%d-A%d-%dx%d-%s" % s)
def test_three_updates_equal_the_host_build_and_a_second_copy(shape):
    T, E, B, epochs = 5, 13, W.BATCH, 2
    batches = [W.make_batch(shape, T, E, seed=s) for s in range(3)]
    perms = [PP.make_perm(T * E, epochs, seed=s) for s in range(3)]
    runs = []
    for _ in range(2):
        model, ppo = device_ppo(shape, T, E, epochs, B, ent_coef=0.01)
        for b, pm in zip(batches, perms):
            ppo.update(fill(ppo, b, pm), shuffle=False)
        runs.append([p.detach().clone() for p in ppo.params()] + ppo.exp_avg + ppo.exp_avg_sq + [ppo.step, ppo.stats, ppo.buffers["workspace"]])
    w, m, v, step = W.fresh_state(W.model_of(shape))
    for b, pm in zip(batches, perms):
        rc, host = W.host_update(w, m, v, step, b, PP.hyper(ent_coef=0.01), pm, B, shape)
        assert rc == 0
    assert int(step[0]) == 3 * epochs * 2
    for x, y, z in zip(runs[0], runs[1], w + m + v + [step, host["stats"], host["workspace"]]):
        assert same_bits(x, y) and same_bits(x, z)
    assert not same_bits(runs[0][0], W.weights_of(W.model_of(shape))[0])               # the updates moved the parameters


def test_all_masked_call_on_the_device():
    shape, T, E = W.SHAPE_A, 5, 13
    b = W.make_batch(shape, T, E)
    b["use"][:] = 0.0
    model, ppo = device_ppo(shape, T, E, 2, 20)
    before = [p.detach().clone() for p in ppo.params()]
    ppo.step.fill_(7)
    g = torch.full((ppo.num_params,), float("nan"), device="cuda")
    ppo.update(fill(ppo, b, PP.make_perm(T * E, 2)), shuffle=False, out_grad=g)
    assert bool((g == 0).all()) and int(ppo.step[0]) == 7 + 8 and ppo.stats.shape == (8, 8)
    assert bool((ppo.stats[:, 3] == 0).all()) and bool((ppo.stats[:, 4] == 1).all())
    for p, p0, m, v in zip(ppo.params(), before, ppo.exp_avg, ppo.exp_avg_sq):
        assert torch.equal(p, p0) and bool((m == 0).all()) and bool((v == 0).all())


def test_out_of_range_perm_entries_on_the_device():
    """a tenth of perm replaced by -1 and N against the same rows taken out through use: the same bits in every output"""
    shape, T, E, B = W.SHAPE_A, 5, 13, 20
    N = T * E
    b = W.make_batch(shape, T, E)
    perm = PP.make_perm(N, 1)
    bad = perm.copy()
    pos = np.random.RandomState(5).permutation(N)[:max(N // 10, 2)]
    bad[0, pos[0::2]] = -1
    bad[0, pos[1::2]] = N
    b0 = dict(b, use=b["use"].copy())
    b0["use"].reshape(-1)[perm[0, pos]] = 0.0
    olp = dev(PP.spread_old_logp(W.model_of(shape), b, PP.hyper()))
    res = []
    for batch, pm in ((b, bad), (b0, perm)):
        model, ppo = device_ppo(shape, T, E, 1, B)
        outs = [torch.full((T, E), float("nan"), device="cuda"), torch.full((T, E), float("nan"), device="cuda"), torch.full((ppo.num_params,), float("nan"), device="cuda")]
        ppo.update(fill(ppo, batch, pm), shuffle=False, old_logp=olp, out_adv=outs[0], out_returns=outs[1], out_grad=outs[2])
        assert int(ppo.step[0]) == 4
        res.append([p.detach().clone() for p in ppo.params()] + ppo.exp_avg + ppo.exp_avg_sq + outs + [ppo.stats])
    for x, y in zip(*res):
        assert bool(torch.isfinite(x).all()) and same_bits(x, y)
    assert float(res[0][-1][:, 4].sum()) == b0["use"].sum()


def test_captured_update_replays_as_eager_updates():
    """update(shuffle=False) captured and replayed three times with shuffle() between the replays, against three eager updates on a twin
    that is handed the same perm: bitwise, and the step count continues"""
    shape, T, E, B = W.SHAPE_A, 5, 40, 64
    batches = [W.make_batch(shape, T, E, seed=s) for s in range(3)]
    model_g, ppo_g = device_ppo(shape, T, E, 2, B)
    model_e, ppo_e = device_ppo(shape, T, E, 2, B)
    assert ppo_g.num_steps == 8 and ppo_g.launches == (4 + 1) * 3 + 2 + 8 * 10
    last = torch.zeros(E, shape[0], device="cuda")
    fill(ppo_g, batches[0], PP.make_perm(T * E, 2))
    ppo_g.grad(last)                             # the kernels are loaded before the capture; the module is not touched
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ppo_g.update(last, shuffle=False)
    for b in batches:
        ppo_g.shuffle()
        pm = ppo_g.perm.cpu().numpy()
        last.copy_(fill(ppo_g, b, pm))
        graph.replay()
        ppo_e.update(fill(ppo_e, b, pm), shuffle=False)
        assert torch.equal(ppo_g.stats, ppo_e.stats)
    torch.cuda.synchronize()
    assert int(ppo_g.step[0]) == int(ppo_e.step[0]) == 24
    for x, y in zip(list(ppo_g.params()) + ppo_g.exp_avg + ppo_g.exp_avg_sq, list(ppo_e.params()) + ppo_e.exp_avg + ppo_e.exp_avg_sq):
        assert same_bits(x, y)


def test_optimizer_round_trip_with_torch_adam_on_the_device():
    shape, T, E = W.SHAPE_ODD, 5, 13
    model, ppo = device_ppo(shape, T, E, 1, W.BATCH)
    opt = torch.optim.Adam(model.parameters(), lr=3e-4, eps=1e-5)
    for _ in range(2):
        opt.zero_grad()
        (model.pi(torch.randn(8, shape[0], device="cuda")).sum() + model.value(torch.randn(8, shape[0], device="cuda")).sum() + model.log_std.sum()).backward()
        opt.step()
    ppo.load_optimizer(opt)
    assert int(ppo.step[0]) == 2 and all(torch.equal(m, opt.state[p]["exp_avg"]) for m, p in zip(ppo.exp_avg, ppo.params()))
    b = W.make_batch(shape, T, E)
    ppo.update(fill(ppo, b, PP.make_perm(T * E, 1)), shuffle=False)
    ppo.export_optimizer(opt)
    assert all(int(opt.state[p]["step"]) == 4 and torch.equal(opt.state[p]["exp_avg_sq"], v) for p, v in zip(ppo.params(), ppo.exp_avg_sq))


@pytest.mark.parametrize("device_normalize", (False, True))
def test_driver_with_the_wide_device_path(device_normalize):
    """a smoke run, not a learning curve"""
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=64, seed=0)
    model, venv, hist = train(env=env, updates=4, algo="ppo", net_arch=(128, 128), activation="relu", device_update=True, device_policy=True,
                              device_normalize=device_normalize, quiet=True, log_every=2)
    assert len(hist) == 2 and model.net_arch == (128, 128) and model.activation == "relu"
    for rec in hist:
        assert all(np.isfinite(v) for v in rec.values()), rec
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_driver_with_the_wide_device_path_under_lazy_auto_reset():
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmPDPickAndPlace-v0", num_envs=64, seed=0, auto_reset="lazy")
    model, venv, hist = train(env=env, updates=4, algo="ppo", net_arch=(128, 128), activation="relu", device_update=True, device_policy=True,
                              device_normalize=True, quiet=True, log_every=4, auto_reset="lazy")
    assert len(hist) == 1 and all(np.isfinite(v) for v in hist[0].values()), hist
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_a2c_device_update_refuses_another_shape():
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=64, seed=0)
    with pytest.raises(ValueError, match="64-64.*a2c_update"):
        train(env=env, updates=1, algo="a2c", net_arch=(128, 128), device_update=True, quiet=True)
    env.close()


def test_wide_device_ppo_learns_reach():
    """dense Reach with [256, 256] tanh towers, the three device flags on.  The bar is half the gain in mean raw reward of the torch block
    at the same sizes and seed, taken once by tools/ppow_rate.py --learn and recorded in profiles/ppow_rate.json: the two
    paths draw different noise."""
    from gym_xarm_amd.train import train
    rec = json.load(open(os.path.join(PH.ROOT, "profiles", "ppow_rate.json")))["learn"]
    model, venv, hist = train("XarmReach-v0", num_envs=rec["num_envs"], updates=rec["updates"], algo="ppo", n_steps=16, net_arch=(256, 256), activation="tanh",
                              config={"reward_type": "dense", "GUI": False}, log_every=rec["updates"] // 2, quiet=True, device_update=True, device_policy=True,
                              device_normalize=True)
    first, last = hist[0]["mean_raw_reward"], hist[-1]["mean_raw_reward"]
    gain = rec["torch"]["last"] - rec["torch"]["first"]
    print("wide device PPO, Reach %d envs x %d updates: mean_raw_reward %.4f -> %.4f (torch block %.4f -> %.4f)"
          % (rec["num_envs"], rec["updates"], first, last, rec["torch"]["first"], rec["torch"]["last"]))
    assert gain > 0 and last - first >= 0.5 * gain, (first, last, rec)
