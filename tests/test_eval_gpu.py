"""Policy evaluation on the MI355X (gym_xarm_amd/evaluation.py DeviceEvaluator, csrc/xarm_k_eval.hip): the three ABI calls against the
host build of the same core bit for bit, whole evaluations against evaluate_policy_torch on a twin env, the captured iteration against
eager runs, the quotas under auto-reset and the EvalCallback inside the drivers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import eval_host as EH
from gym_xarm_amd import evaluation as EV

pytestmark = pytest.mark.gpu


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else x
    return np.ascontiguousarray(x).view(np.uint8).tobytes()


class DeviceState:
    """the ABI calls on torch tensors, with HostEval's surface"""

    def __init__(self, E, N):
        from gym_xarm_amd import _native
        self.L, self.check, self.layout = _native.load(), _native.check, _native.XarmEvalLayout(E, N)
        dev = "cuda"
        self.cur_ret, self.cur_len = torch.full((E,), 7.0, device=dev, dtype=torch.float64), torch.full((E,), 7, device=dev, dtype=torch.int32)
        self.count, self.remaining = torch.full((E,), 7, device=dev, dtype=torch.int32), torch.full((1,), 7, device=dev, dtype=torch.int32)
        self.records, self.out = torch.full((N, 3), 7.0, device=dev, dtype=torch.float64), torch.full((8,), 7.0, device=dev, dtype=torch.float64)

    def _state(self):
        return [C.c_void_p(getattr(self, k).data_ptr()) for k in EH.HostEval.STATE]

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def begin(self):
        self.check(self.L, None, self.L.xarm_eval_begin(C.byref(self.layout), *self._state(), self._stream()), "xarm_eval_begin")

    def step(self, rew, done, success, keep=None):
        t = [None if x is None else torch.from_numpy(x).cuda() for x in (rew, done, success, keep)]
        rc = self.L.xarm_eval_step(C.byref(self.layout), *self._state(), *[None if x is None else C.c_void_p(x.data_ptr()) for x in t], self._stream())
        self.check(self.L, None, rc, "xarm_eval_step")
        torch.cuda.synchronize()

    def summary(self):
        rc = self.L.xarm_eval_summary(C.byref(self.layout), C.c_void_p(self.count.data_ptr()), C.c_void_p(self.records.data_ptr()),
                                      C.c_void_p(self.out.data_ptr()), self._stream())
        self.check(self.L, None, rc, "xarm_eval_summary")
        return self.out


@pytest.mark.parametrize("use_keep", [False, True])
@pytest.mark.parametrize("E,N", EH.SHAPES)
def test_the_three_calls_equal_the_host_build(E, N, use_keep):
    ref, host, dev = EH.Restatement(E, N), EH.HostEval(E, N), DeviceState(E, N)
    host.begin(); dev.begin()

    def same(t=None, wrote=None):
        for k in EH.HostEval.STATE:
            assert bits(getattr(dev, k)) == bits(getattr(host, k)), (k, t)
    same()
    EH.run_to_end(E, N, use_keep, [ref, host, dev], same, extra=10)
    assert int(dev.remaining.item()) == 0 and dev.count.tolist() == ref.target
    assert bits(dev.summary()) == bits(host.summary())


def test_abi_refusals():
    from gym_xarm_amd import _native
    L = _native.load()
    d = DeviceState(4, 4)
    for bad in ((-1, 4), (4, 0)):
        rc = L.xarm_eval_begin(C.byref(_native.XarmEvalLayout(*bad)), *d._state(), None)
        assert rc != 0 and b"xarm_eval_begin" in L.xarm_last_error(None)
    st = d._state()
    assert L.xarm_eval_step(C.byref(d.layout), *st, None, None, None, None, None) != 0 and b"NULL pointer" in L.xarm_last_error(None)
    assert L.xarm_eval_step(C.byref(d.layout), st[0], None, st[2], st[3], st[4], None, None, None, None, None) != 0
    assert L.xarm_eval_summary(C.byref(d.layout), None, st[4], C.c_void_p(d.out.data_ptr()), None) != 0
    assert L.xarm_eval_summary(None, st[2], st[4], C.c_void_p(d.out.data_ptr()), None) != 0
    assert L.xarm_eval_begin(C.byref(_native.XarmEvalLayout(0, 4)), None, None, None, None, None, None) == 0      # no envs: launches nothing


# ---- whole evaluations
def make_norm(env, seed=3):
    """a DeviceVecNormalize for `env` with non-trivial statistics"""
    from gym_xarm_amd.normalize import DeviceVecNormalize
    venv = DeviceVecNormalize(env)
    g = torch.Generator().manual_seed(seed)
    D = venv.dim
    s = venv.stats.cpu()
    s[:D] = torch.randn(D, generator=g, dtype=torch.float64) * 0.3
    s[D:2 * D] = torch.rand(D, generator=g, dtype=torch.float64) * 2.0 + 0.05
    venv.stats.copy_(s)
    return venv


def make_pair(gx, env_id, E, seed=5):
    return gx.make(env_id, num_envs=E, seed=seed), gx.make(env_id, num_envs=E, seed=seed)


@pytest.fixture(scope="module")
def gx():
    import gym_xarm_amd
    return gym_xarm_amd


def check_twin(env, twin, policy, N):
    """DeviceEvaluator.run on env against evaluate_policy_torch on twin: identical records, bit for bit"""
    ev = EV.DeviceEvaluator(env, N)
    res = ev.run(policy)
    ref, rec = EV.evaluate_policy_torch(policy, twin, N, full=True)
    torch.cuda.synchronize()
    assert bits(ev.records) == bits(rec)
    assert res["n_episodes"] == N and ev.count.tolist() == EV.quotas(env.num_envs, N)[0].tolist() and int(ev.remaining.item()) == 0
    assert res["steps"] >= ref["steps"] and res["steps"] % env.max_episode_steps == 0      # the device run reads `remaining` once per check_every steps
    r = rec[:, 0].cpu().numpy()
    assert res["mean_reward"] == pytest.approx(float(np.mean(r)), rel=1e-12, abs=1e-12) and res["std_reward"] == pytest.approx(float(np.std(r)), rel=1e-11, abs=1e-12)
    assert res["success_rate"] == ref["success_rate"] and res["min_reward"] == ref["min_reward"] and res["max_reward"] == ref["max_reward"]
    assert res["mean_length"] == pytest.approx(ref["mean_length"], rel=1e-12)
    assert torch.equal(ev.episode_rewards, ev.records[:, 0]) and torch.equal(ev.episode_lengths, ev.records[:, 1])
    assert np.isfinite(r).all() and (rec[:, 1] >= 1).all()
    return ev, res


@pytest.mark.parametrize("env_id,E,N", [("XarmReach-v0", 64, 100), ("XarmPDPickAndPlace-v0", 64, 64), ("XarmPDHandoverNoGoal-v1", 64, 64)])
def test_device_evaluation_equals_the_torch_evaluator_on_a_twin(gx, env_id, E, N):
    from gym_xarm_amd.device_policy import DevicePolicy
    from gym_xarm_amd.train import ActorCritic
    env, twin = make_pair(gx, env_id, E)
    venv = make_norm(env)
    torch.manual_seed(11)
    model = ActorCritic(venv.dim, env.act_dim).cuda()
    dp = DevicePolicy(model, seed=2)
    policy = EV.as_policy(dp, venv)
    assert policy.kind == "device" and policy.runner is dp
    stats, calls = venv.stats.clone(), dp.calls.clone()
    check_twin(env, twin, policy, N)
    assert torch.equal(stats, venv.stats) and torch.equal(calls, dp.calls)      # frozen statistics, deterministic action
    # the action is the drivers' expression on the normalised row
    obs = env.reset()
    twin.reset()      # the two envs are reset in step
    x = ((EV._flat(obs).double() - venv.obs_mean) / torch.sqrt(venv.obs_var + venv.eps)).clamp(-venv.clip_obs, venv.clip_obs).float()
    with torch.no_grad():
        assert torch.allclose(policy(obs), model.dist(x).mean.clamp(-1, 1), atol=1e-5)
    got, want = EV.evaluate_policy(model, env, 8, normalize=venv), EV.evaluate_policy(model, twin, 8, normalize=venv, backend="torch")
    assert got == pytest.approx(want, rel=1e-11, abs=1e-12)      # the kernel's fixed-order moments against np.mean / np.std
    env.close(); twin.close()


@pytest.mark.parametrize("algo", ["sac", "td3"])
def test_learners_are_normalised_and_deterministic(gx, algo):
    from gym_xarm_amd import sac, td3
    env, twin = make_pair(gx, "XarmReach-v0", 64)
    venv = make_norm(env)
    torch.manual_seed(12)
    model = (sac.SacPolicy if algo == "sac" else td3.Td3Policy)(venv.dim, env.act_dim).cuda()
    policy = EV.as_policy(model, venv)
    assert policy.kind == "device" and type(policy.runner).__name__ == ("DeviceSAC" if algo == "sac" else "DeviceTD3")
    check_twin(env, twin, policy, 100)
    assert int(policy.runner.calls.item()) == 0      # no stochastic call was made
    obs = env.reset()
    x = ((EV._flat(obs).double() - venv.obs_mean) / torch.sqrt(venv.obs_var + venv.eps)).clamp(-venv.clip_obs, venv.clip_obs).float()
    with torch.no_grad():
        want = torch.tanh(model.actor(x)[:, :env.act_dim]) if algo == "sac" else model.action(x)
        assert torch.allclose(policy(obs), want, atol=1e-5)
    env.close(); twin.close()


def test_a_captured_iteration_equals_eager_runs(gx):
    from gym_xarm_amd.train import ActorCritic
    E, N = 130, 200
    env, twin = make_pair(gx, "XarmReach-v0", E)
    venv = make_norm(env)
    torch.manual_seed(13)
    model = ActorCritic(venv.dim, env.act_dim).cuda()
    policy, policy2 = EV.as_policy(model, venv), EV.as_policy(model, venv)
    ev, ev2 = EV.DeviceEvaluator(env, N), EV.DeviceEvaluator(twin, N)
    a, b = ev.run(policy, graph=True), ev2.run(policy2)
    graph = ev._graph
    assert graph is not None and a == b and bits(ev.records) == bits(ev2.records)
    a, b = ev.run(policy, graph=True), ev2.run(policy2)      # the capture is reused
    assert ev._graph is graph and a == b and bits(ev.records) == bits(ev2.records)
    first = ev.records.clone()
    with torch.no_grad():      # in place: the replays read the changed parameters
        for p in model.parameters():
            p.add_(torch.randn_like(p) * 0.3)
    a, b = ev.run(policy, graph=True), ev2.run(policy2)
    assert ev._graph is graph and a == b and bits(ev.records) == bits(ev2.records) and not torch.equal(first, ev.records)
    with pytest.raises(ValueError, match="graph=True"):
        EV.DeviceEvaluator(env, N).run(EV.as_policy(ActorCritic(venv.dim, env.act_dim, (32, 32)).cuda(), venv), graph=True)
    env.close(); twin.close()


def test_quotas_under_auto_reset(gx):
    from gym_xarm_amd.train import ActorCritic
    env = gx.make("XarmReach-v0", num_envs=8, seed=5)
    torch.manual_seed(14)
    model = ActorCritic(env.obs_dim + 2 * env.goal_dim, env.act_dim).cuda()
    ev = EV.DeviceEvaluator(env, 3)
    res = ev.run(EV.as_policy(model))
    assert ev.count.tolist() == [0, 0, 0, 0, 0, 1, 1, 1] and res["n_episodes"] == 3
    assert res["steps"] == env.max_episode_steps      # one read of `remaining`, after one episode length
    assert (ev.episode_lengths <= env.max_episode_steps).all() and (ev.episode_lengths >= 1).all()
    env.close()


@pytest.mark.parametrize("algo", ["a2c", "sac"])
def test_drivers_evaluate_on_the_gpu(algo, tmp_path):
    from gym_xarm_amd import sac
    from gym_xarm_amd.train import train
    if algo == "a2c":
        model, venv, hist = train(env_id="XarmReach-v0", num_envs=64, updates=4, device_normalize=True, device_policy=True, device_update=True,
                                  eval_freq=10, eval_envs=16, log_dir=str(tmp_path), quiet=True, log_every=2)
        calls = 20
    else:
        model, venv, hist = sac.train_sac(env_id="XarmReach-v0", num_envs=64, steps=20, learning_starts=5, batch_size=64, replay="uniform", device_update=True, device_normalize=True,
                                          eval_freq=10, eval_envs=16, log_dir=str(tmp_path), quiet=True, log_every=10)
        calls = 20
    cb = venv.eval_callback
    assert cb.n_calls == calls and cb.device_backend and cb.n_eval_episodes == 16 and cb._policy.kind == "device"
    z = np.load(os.path.join(str(tmp_path), "evaluations.npz"))
    assert z["timesteps"].tolist() == [640, 1280] and z["results"].shape == z["ep_lengths"].shape == z["successes"].shape == (2, 16)
    assert np.isfinite(z["results"]).all() and (z["ep_lengths"] >= 1).all()
    assert os.path.exists(os.path.join(str(tmp_path), "best_eval_model.safetensors")) and cb.saves >= 1
    assert cb.best_mean_reward == pytest.approx(float(np.max(np.mean(z["results"], axis=1))), rel=1e-12, abs=1e-12)
    assert hist[-1]["eval_mean_reward"] == cb.last_mean_reward and hist[-1]["eval_success_rate"] == cb.last_success_rate
    assert all(("eval_mean_reward" in rec) == (rec["env_steps"] >= 640) for rec in hist)


def test_an_evaluation_leaves_the_training_state_alone(gx):
    from gym_xarm_amd.device_policy import DevicePolicy
    from gym_xarm_amd.normalize import DeviceVecNormalize
    from gym_xarm_amd.train import ActorCritic
    env, eval_env = gx.make("XarmReach-v0", num_envs=64, seed=0), gx.make("XarmReach-v0", num_envs=16, seed=1)
    venv = DeviceVecNormalize(env)
    torch.manual_seed(15)
    model = ActorCritic(venv.dim, env.act_dim).cuda()
    dp = DevicePolicy(model, seed=0)
    obs = venv.reset()
    for _ in range(3):
        obs = venv.step(dp.act(obs)["env_action"])[0]
    snap = lambda: (venv.stats.clone(), venv.ret.clone(), dp.calls.clone(), [p.detach().clone() for p in model.parameters()], env.get_state().clone())
    before = snap()
    cb = EV.EvalCallback(eval_env, eval_freq=1, verbose=0)
    cb.on_step(model, venv, 192)
    res = EV.DeviceEvaluator(eval_env, 16).run(EV.as_policy(dp, venv))      # the training DevicePolicy itself, deterministic
    after = snap()
    assert int(before[2].item()) == 3 and res["n_episodes"] == 16 and len(cb.evaluations_results) == 1
    for x, y in zip(before[:3] + (before[4],), after[:3] + (after[4],)):
        assert bits(x) == bits(y)
    assert all(bits(x) == bits(y) for x, y in zip(before[3], after[3]))
    env.close(); eval_env.close()
