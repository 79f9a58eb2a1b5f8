"""The wide device-resident A2C update (csrc/xarm_k_a2cw.hip) through DeviceA2C(wide=True) on the GPU.  Everything the call writes -
returns, the gradient, the stats, the whole workspace, and parameters / square_avg after three real updates - is held to the host build's
BITS (tests/hostbuild_a2cw), and the gradient and the stats to the rule of tests/ppow_host.py against float64 autograd; then the row-count
edges (all 16 row ranges, 17 head groups, head threads that walk two rows, E beside N), the all-masked call, a captured update, a wide
DevicePolicy on the updated module, the driver, and a learning run.  DESIGN.md 26 lists the figures the tests print."""
import json
import os

import numpy as np
import pytest
import torch

import a2c_host as AH
import a2cw_host as AW
import policy_host as PH
import ppow_host as W

pytestmark = pytest.mark.gpu


def device_a2c(shape, T, E, **hyper):
    from gym_xarm_amd.device_a2c import DeviceA2C
    model = W.model_of(shape).cuda()
    a2c = DeviceA2C(model, E, n_steps=T, wide=True, **hyper)
    assert a2c.backend == "wide" and a2c.launches == 3 * shape[3] + 7 == AW.geometry(T, E, shape)["launches"]
    return model, a2c


def fill(a2c, b):
    for k in ("obs", "action", "reward", "done"):
        a2c.buffers[k].copy_(torch.from_numpy(b[k]))
    if b["use"] is None:
        a2c.buffers["use"].fill_(1.0)
    else:
        a2c.buffers["use"].copy_(torch.from_numpy(b["use"]))
    return torch.from_numpy(b["last_obs"]).cuda()


def same_bits(x, y):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x
    y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y
    return x.shape == y.shape and PH.bits(x) == PH.bits(y)


def one_call(shape, T, E, ent, r=None):
    """one lr = 0 call on the device and on the host build: the same bits in every output and in the workspace; then the rule"""
    r = r or AW.reference(shape, T, E, ent)
    model, a2c = device_a2c(shape, T, E, ent_coef=ent, lr=0.0)
    ret, g = torch.full((T, E), float("nan"), device="cuda"), torch.full((a2c.num_params,), float("nan"), device="cuda")
    a2c.update(fill(a2c, r["b"]), out_returns=ret, out_grad=g)
    w, sq = AW.fresh_state(W.model_of(shape))
    rc, host = AW.host_update(w, sq, r["b"], dict(r["h"], lr=0.0), shape)
    assert rc == 0
    assert same_bits(ret, host["returns"]) and same_bits(g, host["grad"]) and same_bits(a2c.stats, host["stats"])
    assert same_bits(a2c.buffers["workspace"], host["workspace"])               # values, returns, activations, deltas, partials, records, grad
    assert all(same_bits(p, a) for p, a in zip(a2c.params(), w)) and all(same_bits(s, a) for s, a in zip(a2c.square_avg, sq))
    ratio, in_y = W.rule(g.cpu().numpy(), r["g64"], r["Y"], r["sizes"])
    print("wide device A2C gradient %s ent %g: Y %.2e, error %.2f Y, error / bound %.3f, settled out %d" % (W.case_id((shape, T, E)), ent, r["Y"], in_y, ratio, r["taken"]))
    assert ratio <= 1.0
    AW.check_stats(a2c.stats.cpu().numpy(), r["st64"], r["Y"], shape[1])
    return a2c, host


@pytest.mark.parametrize("case", AW.CASES, ids=W.case_id)
def test_one_call_equals_the_host_build_and_obeys_the_rule(case):
    shape, T, E = case
    for ent in (0.0, 0.01):
        one_call(shape, T, E, ent)


def test_grad_leaves_the_module_alone_and_equals_update():
    shape, T, E = W.SHAPE_ODD, 5, 13
    r = AW.reference(shape, T, E, 0.01)
    model, a2c = device_a2c(shape, T, E, ent_coef=0.01)
    before = [p.detach().clone() for p in a2c.params()]
    g, ret, st = a2c.grad(fill(a2c, r["b"]))
    w, sq = AW.fresh_state(W.model_of(shape))
    rc, host = AW.host_update(w, sq, r["b"], dict(r["h"], lr=0.0), shape)
    assert rc == 0 and same_bits(g, host["grad"]) and same_bits(ret, host["returns"]) and same_bits(st, host["stats"])
    assert all(torch.equal(p, q) for p, q in zip(a2c.params(), before)) and all(bool((s == 0).all()) for s in a2c.square_avg)


@pytest.mark.parametrize("shape", (W.SHAPE_REF, W.SHAPE_ODD), ids=lambda s: "D%d-A%d-%dx%d-%s" % s)
def test_three_updates_equal_the_host_build_and_a_second_copy(shape):
    T, E = 5, 13
    h = AH.hyper(ent_coef=0.01, gamma=0.95, lr=1e-3)
    batches = [W.make_batch(shape, T, E, seed=s) for s in range(3)]
    runs = []
    for _ in range(2):
        model, a2c = device_a2c(shape, T, E, **h)
        for b in batches:
            a2c.update(fill(a2c, b))
        runs.append([p.detach().clone() for p in a2c.params()] + a2c.square_avg + [a2c.stats, a2c.buffers["workspace"]])
    w, sq = AW.fresh_state(W.model_of(shape))
    for b in batches:
        rc, host = AW.host_update(w, sq, b, h, shape)
        assert rc == 0
    for x, y, z in zip(runs[0], runs[1], w + sq + [host["stats"], host["workspace"]]):
        assert same_bits(x, y) and same_bits(x, z)
    assert not same_bits(runs[0][0], W.weights_of(W.model_of(shape))[0])               # the updates moved the parameters


# ------------------------------------------------------------------------------------------------------------------ row-count edges
def test_all_sixteen_row_ranges_a_one_row_tile_and_seventeen_head_groups():
    shape, T, E = W.SHAPE_A, 1, 4097
    geo = AW.geometry(T, E, shape)
    assert geo["ranges"] == 16 and geo["rows"][16] == 4097 and (4097 - geo["rows"][15]) % 64 == 1 and geo["groups"] == 17
    one_call(shape, T, E, 0.0)


def test_head_threads_that_walk_two_rows():
    """just above 256 HEAD_GROUPS rows, on the 64-64 tanh shape through wide=True (the host build stays quick)"""
    shape, T, E = W.SHAPE_CROSS, 1, 16385
    geo = AW.geometry(T, E, shape)
    assert geo["groups"] == geo["head_groups"] == 64 and T * E == 256 * geo["head_groups"] + 1
    one_call(shape, T, E, 0.01)


def test_bootstrap_forward_carries_its_own_row_count():
    """E = 13 beside N = 65: the bootstrap launches run 13 rows through buffers sized for 65"""
    shape, T, E = W.SHAPE_A, 5, 13
    a2c, host = one_call(shape, T, E, 0.0)
    o = AW.geometry(T, E, shape)["work"]["value"]
    boot = a2c.buffers["workspace"][o + T * E:o + T * E + E].cpu().numpy()
    with torch.no_grad():
        v64 = W.model_of(shape).double().value(torch.from_numpy(AW.reference(shape, T, E, 0.0)["b"]["last_obs"]).double()).numpy()
    assert same_bits(boot, host["boot"]) and np.abs(boot - v64).max() <= 1e-4 * max(1.0, np.abs(v64).max())


def test_all_masked_call_on_the_device():
    shape, T, E = W.SHAPE_REF, 5, 13
    b = W.make_batch(shape, T, E)
    b["use"][:] = 0.0
    model, a2c = device_a2c(shape, T, E)
    before = [p.detach().clone() for p in a2c.params()]
    for s in a2c.square_avg:
        s.uniform_(0.0, 0.01)
    sq0 = [s.clone() for s in a2c.square_avg]
    g = torch.full((a2c.num_params,), float("nan"), device="cuda")
    a2c.update(fill(a2c, b), out_grad=g)
    assert bool((g == 0).all()) and float(a2c.stats[3]) == 0.0 and float(a2c.stats[4]) == 1.0
    alpha = torch.tensor(0.99, dtype=torch.float32, device="cuda")
    for p, p0, s, s0 in zip(a2c.params(), before, a2c.square_avg, sq0):
        assert torch.equal(p, p0) and torch.equal(s, alpha * s0)


def test_captured_update_replays_as_eager_updates():
    """update captured and replayed three times with the buffers rewritten in place, against three eager updates on a twin: bitwise.  The
    chain has no side stream, so the capture has no parallel branches"""
    shape, T, E = W.SHAPE_A, 5, 40
    batches = [W.make_batch(shape, T, E, seed=s) for s in range(3)]
    model_g, a2c_g = device_a2c(shape, T, E, ent_coef=0.01)
    model_e, a2c_e = device_a2c(shape, T, E, ent_coef=0.01)
    last = torch.zeros(E, shape[0], device="cuda")
    fill(a2c_g, batches[0])
    a2c_g.grad(last)                             # the kernels are loaded before the capture; the module is not touched
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a2c_g.update(last)
    for b in batches:
        last.copy_(fill(a2c_g, b))
        graph.replay()
        a2c_e.update(fill(a2c_e, b))
        assert torch.equal(a2c_g.stats, a2c_e.stats)
    torch.cuda.synchronize()
    for x, y in zip(list(a2c_g.params()) + a2c_g.square_avg, list(a2c_e.params()) + a2c_e.square_avg):
        assert same_bits(x, y)
    assert not same_bits(a2c_g.params()[0], W.weights_of(W.model_of(shape))[0])


def test_wide_policy_on_the_updated_module():
    """a wide DevicePolicy on the module the update has written equals the host act call on the updated weights"""
    from gym_xarm_amd.device_policy import DevicePolicy
    shape, T, E = W.SHAPE_REF, 5, 13
    b = W.make_batch(shape, T, E)
    model, a2c = device_a2c(shape, T, E)
    a2c.update(fill(a2c, b))
    pol = DevicePolicy(model, seed=3, wide=True)
    assert pol.backend == "wide"
    rows = np.random.RandomState(0).uniform(-2.5, 2.5, (33, shape[0])).astype(np.float32)
    out = pol.act(torch.from_numpy(rows).cuda())
    w = [p.detach().cpu().numpy() for p in a2c.params()]
    host = W.host_act([PH.aligned(a) for a in w], rows, shape, seed=3)
    for k in ("action", "env_action", "logp", "value"):
        assert same_bits(out[k], host[k]), k
    assert not same_bits(w[0], W.weights_of(W.model_of(shape))[0])


def test_optimizer_round_trip_with_torch_rmsprop_on_the_device():
    shape, T, E = W.SHAPE_ODD, 5, 13
    model, a2c = device_a2c(shape, T, E)
    opt = torch.optim.RMSprop(model.parameters(), lr=7e-4, alpha=0.99, eps=1e-5)
    for _ in range(2):
        opt.zero_grad()
        (model.pi(torch.randn(8, shape[0], device="cuda")).sum() + model.value(torch.randn(8, shape[0], device="cuda")).sum() + model.log_std.sum()).backward()
        opt.step()
    a2c.load_optimizer(opt)
    assert len(a2c.square_avg) == 17 and all(torch.equal(s, opt.state[p]["square_avg"]) for s, p in zip(a2c.square_avg, a2c.params()))
    a2c.update(fill(a2c, W.make_batch(shape, T, E)))
    a2c.export_optimizer(opt)
    assert all(torch.equal(opt.state[p]["square_avg"], s) for p, s in zip(a2c.params(), a2c.square_avg))


# ----------------------------------------------------------------------------------------------------------------------- driver
@pytest.mark.parametrize("device_normalize", (False, True))
def test_driver_with_the_wide_device_path(device_normalize):
    """a smoke run, not a learning curve"""
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=64, seed=0)
    model, venv, hist = train(env=env, updates=4, algo="a2c", net_arch=(128, 128), activation="relu", device_update=True, device_policy=True,
                              device_normalize=device_normalize, wide=True, quiet=True, log_every=2)
    assert len(hist) == 2 and model.net_arch == (128, 128) and model.activation == "relu"
    for rec in hist:
        assert all(np.isfinite(v) for v in rec.values()), rec
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_driver_with_the_wide_device_path_under_lazy_auto_reset():
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmPDPickAndPlace-v0", num_envs=64, seed=0, auto_reset="lazy")
    model, venv, hist = train(env=env, updates=4, algo="a2c", net_arch=(128, 128), activation="relu", device_update=True, device_policy=True,
                              device_normalize=True, wide=True, quiet=True, log_every=4, auto_reset="lazy")
    assert len(hist) == 1 and all(np.isfinite(v) for v in hist[0].values()), hist
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_driver_runs_the_reference_shape_without_the_other_device_flags():
    import gym_xarm_amd
    from gym_xarm_amd.train import train
    env = gym_xarm_amd.make("XarmReach-v0", num_envs=64, seed=0)
    model, venv, hist = train(env=env, updates=2, algo="a2c", net_arch=(256, 256, 256), activation="relu", device_update=True, wide=True, gamma=0.95, lr=1e-3,
                              quiet=True, log_every=2)
    assert len(hist) == 1 and all(np.isfinite(v) for v in hist[0].values()) and all(bool(torch.isfinite(p).all()) for p in model.parameters())


def test_wide_device_a2c_learns_reach():
    """dense Reach with [256, 256] tanh towers, A2C's defaults, the three device flags on, wide=True.  The bar is half the gain in mean raw
    reward of the torch block at the same sizes and seed, taken once by tools/a2cw_rate.py --learn and recorded in profiles/a2cw_rate.json
    (DESIGN.md 26): the two paths draw different noise."""
    from gym_xarm_amd.train import train
    rec = json.load(open(os.path.join(PH.ROOT, "profiles", "a2cw_rate.json")))["learn"]
    model, venv, hist = train("XarmReach-v0", num_envs=rec["num_envs"], updates=rec["updates"], algo="a2c", net_arch=(256, 256), activation="tanh",
                              config={"reward_type": "dense", "GUI": False}, log_every=rec["updates"] // 2, quiet=True, device_update=True, device_policy=True,
                              device_normalize=True, wide=True)
    first, last = hist[0]["mean_raw_reward"], hist[-1]["mean_raw_reward"]
    gain = rec["torch"]["last"] - rec["torch"]["first"]
    print("wide device A2C, Reach %d envs x %d updates: mean_raw_reward %.4f -> %.4f (torch block %.4f -> %.4f)"
          % (rec["num_envs"], rec["updates"], first, last, rec["torch"]["first"], rec["torch"]["last"]))
    assert gain > 0 and last - first >= 0.5 * gain, (first, last, rec)
