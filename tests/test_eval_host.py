"""CPU tests of policy evaluation: the g++ build of csrc/xarm_eval_core.h against a plain-Python restatement of the
semantics, its summary against the same fixed-order algorithm in NumPy and against np.mean / np.std, evaluate_policy_torch, the
EvalCallback inside the three drivers and the two CLIs on scripted host envs."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import eval_host as EH
from gym_xarm_amd import evaluation as EV


@pytest.mark.parametrize("use_keep", [False, True])
@pytest.mark.parametrize("E,N", EH.SHAPES)
def test_host_build_is_the_restatement(E, N, use_keep):
    ref, host = EH.Restatement(E, N), EH.HostEval(E, N)
    host.begin()
    assert host.remaining[0] == N and not host.records.any() and not host.count.any() and not host.cur_ret.any() and not host.cur_len.any()
    seen = {"before": N, "frozen": None}

    def after_step(t, wrote):
        assert host.remaining[0] == seen["before"] - wrote == ref.remaining      # falls by exactly the records written in the step
        seen["before"] = int(host.remaining[0])
        assert host.count.tolist() == ref.count and host.cur_len.tolist() == ref.cur_len and host.cur_ret.tolist() == ref.cur_ret
        assert host.records.tolist() == ref.records
        if ref.remaining == 0:
            if seen["frozen"] is not None:      # the further steps change neither the records nor the counts
                assert np.array_equal(seen["frozen"][0], host.records) and np.array_equal(seen["frozen"][1], host.count)
            seen["frozen"] = (host.records.copy(), host.count.copy())
    steps = EH.run_to_end(E, N, use_keep, [ref, host], after_step, extra=10)
    assert host.count.tolist() == ref.target == [(N + i) // E for i in range(E)] and sum(ref.target) == N
    L = EH.lib()
    assert [L.eh_target(C.byref(host.layout), i) for i in range(E)] == ref.target
    assert [L.eh_base(C.byref(host.layout), i) for i in range(E)] == ref.base
    t, b = EV.quotas(E, N)
    assert t.tolist() == ref.target and b.tolist() == ref.base
    # every record is an episode of the scripted stream: its length is the env's (kept steps only), its return the kept rewards' sum
    lens = EH.ep_lens(E)
    for i in range(E):
        for k in range(ref.target[i]):
            assert host.records[ref.base[i] + k, 1] == lens[i]
    assert steps >= 10 + max(lens[i] * ref.target[i] for i in range(E))


def test_a_masked_step_adds_neither_reward_nor_length():
    host = EH.HostEval(3, 3)
    host.begin()
    rew, z = np.array([1.5, 2.5, 3.5], np.float32), np.zeros(3, np.uint8)
    host.step(rew, z, z, np.array([1, 0, 1], np.uint8))
    assert host.cur_ret.tolist() == [1.5, 0.0, 3.5] and host.cur_len.tolist() == [1, 0, 1]
    host.step(rew, np.array([0, 1, 1], np.uint8), np.array([0, 1, 0], np.uint8), np.array([0, 1, 1], np.uint8))
    assert host.cur_ret.tolist() == [1.5, 0.0, 0.0] and host.cur_len.tolist() == [1, 0, 0]
    assert host.records.tolist() == [[0.0, 0.0, 0.0], [2.5, 1.0, 1.0], [7.0, 2.0, 0.0]] and host.remaining[0] == 1


@pytest.mark.parametrize("E,N", EH.SHAPES + ((64, 4096),))
def test_summary_is_the_fixed_order_algorithm_and_numpys_moments(E, N):
    ref, host = EH.Restatement(E, N), EH.HostEval(E, N)
    host.begin()
    out = host.summary().copy()
    assert out[7] == 0.0 and np.isnan(out[:7]).all()      # before any record: n_episodes 0 and NaN means, as np.mean([])
    state = {"mid": None}

    def after_step(t, wrote):
        if state["mid"] is None and 0 < ref.remaining < N:      # part of the slots written: they are told apart by the count
            state["mid"] = True
            w = ref.written()
            assert np.array_equal(host.summary(), EH.summary_fixed_order(ref.records, w), equal_nan=True)
            assert host.out[7] == sum(w) == N - ref.remaining
    EH.run_to_end(E, N, False, [ref, host], after_step, extra=0)
    out = host.summary().copy()
    assert np.array_equal(out, EH.summary_fixed_order(ref.records, [True] * N))
    r, l, s = (np.asarray(x, np.float64) for x in ref.lists())
    if N > 1:
        assert np.std(r) >= 0.1 * abs(np.mean(r))
    assert out[0] == pytest.approx(np.mean(r), rel=1e-12, abs=1e-300) and out[1] == pytest.approx(np.std(r), rel=1e-11, abs=1e-300)
    assert out[2] == pytest.approx(np.mean(l), rel=1e-12) and out[3] == pytest.approx(np.std(l), rel=1e-11, abs=1e-300)
    assert out[4] == np.mean(s) and out[5] == r.min() and out[6] == r.max() and out[7] == N


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("E,N", [(3, 7), (8, 3), (65, 100), (5, 5)])
def test_evaluate_policy_torch_returns_the_restatements_lists(E, N, lazy):
    ref, steps = EH.expected_lists(E, N, lazy)
    env = EH.StreamEnv(E, lazy=lazy)
    policy = lambda obs: torch.zeros(E, env.act_dim)
    res, rec = EV.evaluate_policy_torch(policy, env, N, full=True)
    r, l, s = ref.lists()
    assert rec[:, 0].tolist() == r and rec[:, 1].tolist() == l and rec[:, 2].tolist() == s      # env-major, bit for bit
    assert res["steps"] == steps and res["n_episodes"] == N
    assert res["mean_reward"] == float(np.mean(r)) and res["std_reward"] == float(np.std(r))
    assert res["mean_length"] == float(np.mean(l)) and res["success_rate"] == float(np.mean(s))
    assert res["min_reward"] == min(r) and res["max_reward"] == max(r)
    assert EV.evaluate_policy(policy, EH.StreamEnv(E, lazy=lazy), N) == (float(np.mean(r)), float(np.std(r)))      # SB3's return, backend "torch" on a CPU env
    assert EV.evaluate_policy(policy, EH.StreamEnv(E, lazy=lazy), N, return_episode_rewards=True) == (r, l)
    if N < E:      # the first E - N envs contribute nothing
        assert ref.target[:E - N] == [0] * (E - N) and ref.target[E - N:] == [1] * N


def test_evaluate_policy_threshold_and_refusals():
    env = EH.StreamEnv(3)
    policy = lambda obs: torch.zeros(3, env.act_dim)
    mean, _ = EV.evaluate_policy(policy, env, 7)
    EV.evaluate_policy(policy, EH.StreamEnv(3), 7, reward_threshold=mean - 0.5)
    with pytest.raises(AssertionError, match="Mean reward below threshold"):
        EV.evaluate_policy(policy, EH.StreamEnv(3), 7, reward_threshold=mean + 0.5)
    for n in (0, -2):
        with pytest.raises(ValueError, match="n_eval_episodes must be >= 1"):
            EV.evaluate_policy(policy, EH.StreamEnv(3), n)
        with pytest.raises(ValueError, match="n_eval_episodes must be >= 1"):
            EV.evaluate_policy_torch(policy, EH.StreamEnv(3), n)
    with pytest.raises(ValueError, match="backend must be"):
        EV.evaluate_policy(policy, EH.StreamEnv(3), 3, backend="numpy")


def test_layout_refusals_and_the_cpu_refusal():
    from gym_xarm_amd import _native
    L = EH.lib()
    st = [np.zeros(8), np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(1, np.int32), np.zeros((8, 3))]
    for bad in ((-1, 4), (4, 0), (4, -3)):
        lay = _native.XarmEvalLayout(*bad)
        assert L.eh_begin(C.byref(lay), *[EH._p(x) for x in st]) == -1
        assert L.eh_summary(C.byref(lay), EH._p(st[2]), EH._p(st[4]), EH._p(np.zeros(8))) == -1
    assert L.eh_begin(None, *[EH._p(x) for x in st]) == -1
    assert L.eh_begin(C.byref(_native.XarmEvalLayout(0, 4)), *[EH._p(x) for x in st]) == 0      # no envs: nothing to do
    assert C.sizeof(_native.XarmEvalLayout) == 8
    with pytest.raises(ValueError, match="evaluate_policy_torch is the torch implementation"):
        EV.DeviceEvaluator(EH.StreamEnv(3), 3)
    with pytest.raises(ValueError, match="n_eval_episodes must be >= 1"):
        EV.DeviceEvaluator(EH.StreamEnv(3), 0)


def test_as_policy_takes_the_drivers_expressions_on_a_cpu_model():
    from gym_xarm_amd import sac, td3
    from gym_xarm_amd.train import ActorCritic, VecNormalize
    torch.manual_seed(0)
    env = EH.StreamEnv(4)
    venv = VecNormalize(env)
    for _ in range(3):
        venv._norm(venv._flat(env._obs()) * 3.0 + 1.0)      # non-trivial statistics
    before = (venv.obs_rms.mean.clone(), venv.obs_rms.var.clone(), venv.obs_rms.count)
    obs = env.reset()
    x = ((venv._flat(obs) - venv.obs_rms.mean) / torch.sqrt(venv.obs_rms.var + venv.eps)).clamp(-venv.clip_obs, venv.clip_obs)
    ac, sp, tp = ActorCritic(venv.dim, 2), sac.SacPolicy(venv.dim, 2), td3.Td3Policy(venv.dim, 2)
    with torch.no_grad():
        assert torch.equal(EV.as_policy(ac, venv)(obs), ac.dist(x).mean.clamp(-1, 1))
        assert torch.equal(EV.as_policy(sp, venv)(obs), torch.tanh(sp.actor(x)[:, :2]))
        assert torch.equal(EV.as_policy(tp, venv)(obs), tp.action(x))
        assert torch.equal(EV.as_policy(ac)(obs), ac.dist(venv._flat(obs)).mean.clamp(-1, 1))      # no normaliser: the raw row
    assert EV.as_policy(ac, venv).kind == "torch"
    f = lambda o: None
    assert EV.as_policy(f) is f                                                                  # any callable is passed through
    assert torch.equal(before[0], venv.obs_rms.mean) and torch.equal(before[1], venv.obs_rms.var) and before[2] == venv.obs_rms.count
    with pytest.raises(TypeError):
        EV.as_policy(3)


def _driver(algo, tmp_path, **kw):
    from gym_xarm_amd import sac, td3
    from gym_xarm_amd.train import train
    if algo in ("a2c", "ppo"):
        return train(env_id="Scripted-v0", updates=6, n_steps=5, log_every=3, quiet=True, env=EH.StreamEnv(6), algo=algo,
                     log_dir=None if tmp_path is None else str(tmp_path), **kw)
    fn = sac.train_sac if algo == "sac" else td3.train_td3
    return fn(env=EH.StreamEnv(6), steps=30, learning_starts=5, batch_size=16, quiet=True, log_every=15, replay="uniform", buffer_size=120,
              log_dir=None if tmp_path is None else str(tmp_path), **kw)


@pytest.mark.parametrize("algo", ["a2c", "ppo", "sac", "td3"])
def test_drivers_evaluate_every_eval_freq_steps(algo, tmp_path):
    E_eval, N, k = 5, 7, 10
    eval_env = EH.StreamEnv(E_eval)
    model, venv, hist = _driver(algo, tmp_path, eval_freq=k, n_eval_episodes=N, eval_env=eval_env)
    cb = venv.eval_callback
    n = 30 // k
    assert isinstance(cb, EV.EvalCallback) and cb.n_calls == 30 and len(cb.evaluations_timesteps) == n and eval_env.closed
    z = np.load(os.path.join(str(tmp_path), "evaluations.npz"))
    assert sorted(z.files) == ["ep_lengths", "results", "successes", "timesteps"]
    assert z["timesteps"].tolist() == [6 * k * (j + 1) for j in range(n)]
    assert z["results"].shape == z["ep_lengths"].shape == z["successes"].shape == (n, N)
    ref, _ = EH.expected_lists(E_eval, N)      # the scripted env's episodes do not depend on the actions: every evaluation sees these
    r, l, s = ref.lists()
    for j in range(n):
        assert z["results"][j].tolist() == r and z["ep_lengths"][j].tolist() == l and z["successes"][j].tolist() == s
    assert cb.last_mean_reward == cb.best_mean_reward == float(np.mean(r)) and cb.last_success_rate == float(np.mean(s))
    assert cb.saves == 1 and os.path.exists(os.path.join(str(tmp_path), "best_eval_model.safetensors"))      # saved at the first evaluation only: no later one improved
    assert not os.path.exists(os.path.join(str(tmp_path), "best_model.safetensors"))      # the training-reward callback's file: it never fell due
    assert all(rec["eval_mean_reward"] == float(np.mean(r)) and rec["eval_success_rate"] == float(np.mean(s)) for rec in hist)
    from gym_xarm_amd import sac, td3, train
    load = {"a2c": train.load_checkpoint, "ppo": train.load_checkpoint, "sac": sac.load_checkpoint, "td3": td3.load_checkpoint}[algo]
    loaded, vn = load(cb.save_path)
    assert set(loaded.state_dict()) == set(model.state_dict()) and "obs_mean" in vn


@pytest.mark.parametrize("algo", ["a2c", "ppo", "sac", "td3"])
def test_drivers_without_eval_freq_build_nothing(algo, tmp_path):
    model, venv, hist = _driver(algo, tmp_path)
    assert not hasattr(venv, "eval_callback")
    assert not os.path.exists(os.path.join(str(tmp_path), "evaluations.npz"))
    assert not os.path.exists(os.path.join(str(tmp_path), "best_eval_model.safetensors"))
    assert not any(k.startswith("eval_") for rec in hist for k in rec)
    _, venv2, hist2 = _driver(algo, None, eval_freq=1000, eval_env=EH.StreamEnv(3))      # on, but no evaluation fell due: the keys wait for one
    assert [sorted(rec) for rec in hist2] == [sorted(rec) for rec in hist] and venv2.eval_callback.evaluations_timesteps == []


def test_callback_defaults_to_one_episode_per_eval_env_and_counts_calls(tmp_path):
    from gym_xarm_amd.train import ActorCritic, VecNormalize
    env = EH.StreamEnv(4)
    venv, model = VecNormalize(env), ActorCritic(11, 2)
    cb = EV.EvalCallback(EH.StreamEnv(9), eval_freq=3, log_dir=str(tmp_path), verbose=0)
    assert cb.n_eval_episodes == 9
    for i in range(7):
        assert cb.on_step(model, venv, 100 * (i + 1)) is True
    assert cb.evaluations_timesteps == [300, 600] and np.asarray(cb.evaluations_results).shape == (2, 9) and cb.saves == 1
    with pytest.raises(ValueError):
        EV.EvalCallback(EH.StreamEnv(2), eval_freq=0)


def test_both_clis_have_the_options(tmp_path, capsys):
    from gym_xarm_amd import train
    from gym_xarm_amd.train import ActorCritic, VecNormalize, save_model
    with pytest.raises(SystemExit):
        train.main(["--eval-episodes", "5"])                        # needs --eval-freq
    with pytest.raises(SystemExit):
        train.main(["--eval-freq", "ten"])
    with pytest.raises(SystemExit):
        EV.main(["--env", "XarmReach-v0"])                          # --checkpoint is required
    with pytest.raises(SystemExit):
        EV.main(["--checkpoint", "x", "--algo", "dqn"])
    # the evaluation CLI round-trips a checkpoint written by save_model
    torch.manual_seed(1)
    env = EH.StreamEnv(4)
    venv = VecNormalize(env)
    venv._norm(venv._flat(env._obs()) * 2.0)
    model = ActorCritic(venv.dim, env.act_dim)
    path = os.path.join(str(tmp_path), "agent.safetensors")
    save_model(path, model, venv)
    assert EV.checkpoint_algo(path) == "a2c"
    eval_env = EH.StreamEnv(4)
    res = EV.main(["--checkpoint", path, "--env", "Scripted-v0", "--num-envs", "4", "--episodes", "6"], env=eval_env)
    printed = __import__("json").loads(capsys.readouterr().out.strip().splitlines()[-1])
    ref, steps = EH.expected_lists(4, 6)
    r, l, s = ref.lists()
    assert printed["mean_reward"] == res["mean_reward"] == float(np.mean(r)) and printed["n_episodes"] == 6 and printed["steps"] == steps
    assert printed["success_rate"] == float(np.mean(s)) and printed["algo"] == "a2c" and printed["deterministic"] is True and eval_env.closed
    # the actions the CLI fed the env are the loaded model's deterministic ones under the file's statistics
    twin, tv = EH.StreamEnv(4), VecNormalize(EH.StreamEnv(4))
    tv.load_state_dict({k: v for k, v in venv.state_dict().items()})
    pol = EV.as_policy(model, tv)
    obs = twin.reset()
    assert torch.equal(eval_env.actions[0], pol(obs))
    from gym_xarm_amd import sac, td3
    for cls, name in ((sac.SacPolicy, "sac"), (td3.Td3Policy, "td3")):
        p2 = os.path.join(str(tmp_path), name + ".safetensors")
        save_model(p2, cls(venv.dim, env.act_dim), venv)
        assert EV.checkpoint_algo(p2) == name
        out = EV.main(["--checkpoint", p2, "--episodes", "4", "--stochastic"], env=EH.StreamEnv(4))
        assert out["algo"] == name and out["n_episodes"] == 4 and out["deterministic"] is False
