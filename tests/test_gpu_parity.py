"""Parity tests proper (MI355X): every call goes through the C ABI (include/xarm_hip.h) via
gym_xarm_amd and is compared with the CPU oracle / the committed golden fixtures.  Floating point
path: tolerance = atol 5e-4 + rtol 2e-4 + K x oracle-sensitivity (oracle/parity.py), integer/flag
outputs exact wherever the transition is well conditioned, sparse rewards bit-exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gx():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gym_xarm_amd
    return gym_xarm_amd


def _np(t):
    return t.detach().cpu().numpy()


class _Maker:
    """gx.make with the PickAndPlace kernel family pinned: 'lane' = one env per lane for step and reset (k_step /
    k_reset), 'coop' = the 16-lanes-per-env kernels (k_step_coop / k_reset_coop, the default for the batch sizes of
    these tests), 'fast' = what a 65 536-env batch steps on by default: the pad-free fast kernel with the hand-off of the
    envs that have an active finger-pad row to the cooperative kernel (k_step_fast_stage + k_step_coop_list_stage), resets on k_reset"""

    def __init__(self, gx, family):
        self.gx, self.family, self.vec_env = gx, family, gx.vec_env

    def make(self, env_id, **kw):
        if self.family == "lane":
            kw.setdefault("step_coop_limit", -1)
            kw.setdefault("reset_coop_limit", -1)
        if self.family == "fast":
            kw.setdefault("step_coop_limit", 1)       # every batch of more than one env is "large": the fast pipeline
            kw.setdefault("reset_coop_limit", -1)
        return self.gx.make(env_id, **kw)


@pytest.fixture(scope="module", params=["lane", "coop", "fast"])
def gxk(request, gx):
    return _Maker(gx, request.param)


def test_native_library_is_loaded(gx):
    """the product path maps libxarm_hip.so and nothing of the oracle (fresh interpreter: other test modules of this
    session load the oracle as their checker)"""
    import subprocess, sys
    code = ("import sys; sys.path.insert(0, %r); import gym_xarm_amd\n"
            "env = gym_xarm_amd.make('XarmPDPickAndPlace-v0', num_envs=64); env.reset(); env.step(__import__('torch').zeros(64, 4))\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert 'libxarm_hip.so' in maps and 'libxarm_oracle' not in maps and 'libxarm_host' not in maps\n"
            "print('native ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "native ok" in out.stdout, out.stderr[-2000:]
    env = gx.make("XarmPDPickAndPlace-v0", num_envs=64)
    assert "libxarm_hip.so" in open("/proc/self/maps").read()
    env.close()


def test_init_and_reset_match_oracle(gxk, oracle, parity):
    E = 256
    kw = dict(init_grasp_rate=0.25, goal_ground_rate=0.5)
    env = gxk.make("XarmPDPickAndPlace-v0", num_envs=E, seed=21, auto_reset=False,
                  config=dict(gxk.vec_env.CONFIG_DEFAULTS, **kw))
    ora = oracle.OraclePnP(E, seed=21, **kw)
    np.testing.assert_allclose(_np(env.get_state()), ora.state, atol=1e-6)
    obs = env.reset()
    o_obs, o_ag, o_dg = ora.reset()
    st = _np(env.get_state()).astype(np.float64)
    # reset = 6 ticks from the zero pose: compare where the object does not start inside the fingers
    clean = np.abs(ora.state[:, 19]) > 0.09
    assert clean.mean() > 0.3
    np.testing.assert_allclose(st[clean, :31], ora.state[clean, :31], atol=3e-3)
    np.testing.assert_allclose(_np(obs["desired_goal"]), o_dg, atol=1e-6)
    assert (st[:, 52] == 0).all() and (st[:, 53] == 1).all()
    env.close()


@pytest.mark.parametrize("key,seed", [("rand", 7), ("grasp", 1)])
def test_step_replays_golden_rollout(gxk, golden_rollout, parity, key, seed):
    g = golden_rollout
    S, A = g[key + "_states"], g[key + "_actions"]
    E = S.shape[1]
    env = gxk.make("XarmPDPickAndPlace-v0", num_envs=E, seed=seed, auto_reset=False)
    n_flag, n_all = 0, 0
    for t in range(A.shape[0]):
        env.set_state(S[t])
        obs, rew, done, info = env.step(torch.tensor(A[t], dtype=torch.float32))
        st = _np(env.get_state()).astype(np.float64)
        sens = g[key + "_sens"][t]
        parity.compare(st[:, parity.CONT], S[t + 1][:, parity.CONT], sens, what="%s t=%d" % (key, t),
                       frac_tight=0.9 if key == "rand" else 0.75, max_exempt=0.15 if key == "rand" else 0.25)   # grasp: 4 envs, one may sit on a discontinuity
        ok = sens < 1e-3
        np.testing.assert_allclose(_np(obs["observation"])[ok], g[key + "_obs"][t][ok], atol=2e-3)
        assert np.array_equal(_np(rew)[ok], g[key + "_rew"][t][ok].astype(np.float32))   # sparse reward: exact
        assert np.array_equal(_np(done)[ok], g[key + "_done"][t][ok])
        assert np.array_equal(_np(info["is_success"])[ok], g[key + "_succ"][t][ok])
        assert (st[:, 52] == S[t + 1][:, 52]).all()
        n_flag += (st[ok, 50] == S[t + 1][ok, 50]).sum()
        n_all += ok.sum()
    assert n_flag >= 0.98 * n_all     # touch flag (dist < 0.02 threshold) may flip on exact ties only
    env.close()


def test_live_oracle_rollout_with_sensitivity(gxk, oracle, parity):
    """fresh seeds, 512 envs, 6 steps after reset: HIP vs oracle from identical injected states"""
    E = 512
    env = gxk.make("XarmPDPickAndPlace-v0", num_envs=E, seed=99, auto_reset=False)
    ora = oracle.OraclePnP(E, seed=99)
    env.reset()
    gen = torch.Generator().manual_seed(3)
    for t in range(6):
        st0 = _np(env.get_state()).astype(np.float64)
        a = torch.rand(E, 4, generator=gen) * 2 - 1
        obs, rew, done, info = env.step(a)
        r = parity.oracle_step_with_sens(ora, st0, a.numpy().astype(np.float64), seed=t)
        nxt, o_obs, o_ag, o_dg, o_rew, o_done, o_succ, sens = r
        st = _np(env.get_state()).astype(np.float64)
        stats = parity.compare(st[:, parity.CONT], nxt[:, parity.CONT], sens, what="live t=%d" % t, frac_tight=0.9, max_exempt=0.1)
        ok = sens < 1e-3
        assert np.array_equal(_np(rew)[ok], o_rew[ok].astype(np.float32))
        assert np.array_equal(_np(done)[ok], o_done[ok])
        np.testing.assert_allclose(_np(obs["achieved_goal"])[ok], o_ag[ok], atol=1e-3)
    env.close()


def test_substep_hook_matches_oracle_tick(gx, oracle):
    """15 substeps toward the current pose == one oracle env step with a zero action from a
    settled state (IK target == current EEF, finger target == current finger)"""
    E = 64
    env = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=5, auto_reset=False)
    env.reset()
    for _ in range(30):
        env.step(torch.zeros(E, 4))
    st0 = _np(env.get_state()).astype(np.float64)
    qt = st0[:, :9].copy()
    qt[:, 7:] = np.clip(st0[:, 7:8], 0.01, 0.04)
    env.debug_substeps(torch.tensor(qt, dtype=torch.float32), 15)
    st = _np(env.get_state()).astype(np.float64)
    far = np.abs(st0[:, 19]) > 0.09
    np.testing.assert_allclose(st[far, :9], st0[far, :9], atol=2e-4)          # holds its pose
    z = st[far, 20]                                                           # rests upright (0.04) or tipped over (0.025)
    assert (np.minimum(np.abs(z - 0.04), np.abs(z - 0.025)) < 2e-3).all()
    env.close()


def test_compute_reward_bit_exact_against_reference_golden(gx, golden_reward):
    g = golden_reward
    ag32, g32 = g["achieved_goal"].astype(np.float32), g["goal"].astype(np.float32)
    d32 = np.sqrt(((ag32 - g32) ** 2).sum(1, dtype=np.float32))
    for rt in ("sparse", "dense_o2g"):
        env = gx.make("XarmPDPickAndPlace-v0", num_envs=64, config=dict(gx.vec_env.CONFIG_DEFAULTS, reward_type=rt))
        out = _np(env.compute_reward(torch.tensor(ag32), torch.tensor(g32)))
        ref = g["reward_" + rt]
        if rt == "sparse":
            edge = np.abs(np.linalg.norm(g["achieved_goal"] - g["goal"], axis=1) - 0.05) < 1e-6   # fp32 ties
            assert np.array_equal(out[~edge], ref[~edge].astype(np.float32))
            assert set(np.unique(out)) <= {0.0, 1.0}
        else:
            np.testing.assert_allclose(out, ref, atol=1e-6)
        # batch shapes as HER uses them
        out2 = _np(env.compute_reward(torch.tensor(ag32).reshape(8, 64, 3), torch.tensor(g32).reshape(8, 64, 3)))
        assert out2.shape == (8, 64) and np.array_equal(out2.reshape(-1), out)
        assert _np(env.compute_reward(torch.zeros(0, 3), torch.zeros(0, 3))).shape == (0,)
        env.close()


def test_spaces_rollout_like_reference_test_py(gx):
    """the reference's only test pattern (test.py:16-29): random rollout with space containment"""
    env = gx.make("XarmPickAndPlace-v1", config=dict(GUI=False, num_obj=1, reward_type="sparse", init_grasp_rate=0.0,
                                                      goal_ground_rate=0.0, goal_shape="air"))
    ob = env.reset()
    for i in range(env._max_episode_steps + 5):
        assert env.observation_space.contains(ob)
        a = env.action_space.sample()
        assert env.action_space.contains(a)
        ob, r, done, info = env.step(a)
        assert ob["observation"].shape == (24,) and ob["observation"].dtype == np.float32
        assert isinstance(r, float) and isinstance(done, bool) and info["is_success"].shape == (1,)
        if done:
            assert i + 1 == env._max_episode_steps or info["is_success"][0] == 1.0
            ob = env.reset()
    with pytest.raises(AssertionError, match="action shape error"):
        env.step(np.zeros(3))
    env.close()


def test_auto_reset_semantics(gxk):
    E = 128
    env = gxk.make("XarmPDPickAndPlace-v0", num_envs=E, seed=8)
    env.reset()
    st = env.get_state()
    st[:32, 52] = 49                       # these finish on the next step
    env.set_state(st)
    obs, rew, done, info = env.step(torch.zeros(E, 4))
    d = _np(done).astype(bool)
    assert d[:32].all() and np.array_equal(d[32:], _np(info["is_success"])[32:].astype(bool))
    d[32:] = False
    s = _np(env.get_state())
    assert (s[:32, 52] == 0).all() and (s[:32, 53] == 2).all()        # fresh episode
    live = ~_np(done).astype(bool)
    assert (s[live, 52] == 1).all() and (s[live, 53] == 1).all()
    assert _np(info["TimeLimit.truncated"])[:32].all()
    term = _np(info["terminal_observation"])
    assert np.abs(term[:32] - _np(obs["observation"])[:32]).max() > 1e-3   # obs rows hold the NEW episode
    np.testing.assert_allclose(_np(obs["achieved_goal"])[:32], s[:32, 18:21], atol=0)
    np.testing.assert_allclose(_np(obs["desired_goal"]), s[:, 31:34], atol=0)
    # masked reset through the ABI
    m = torch.zeros(E, dtype=torch.uint8)
    m[100:] = 1
    env.reset(mask=m)
    s2 = _np(env.get_state())
    assert (s2[100:, 53] == s[100:, 53] + 1).all() and np.array_equal(s2[:100], s[:100])
    env.close()


def test_full_size_properties_65536(gx):
    """BASELINE size: size-independent properties (determinism, shard invariance, invariants)"""
    E = 65536
    a = [torch.rand(E, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(k)) * 2 - 1 for k in range(3)]

    def run(n, off):
        env = gx.make("XarmPDPickAndPlace-v0", num_envs=n, seed=17, env_id_offset=off)
        env.reset()
        for k in range(3):
            obs, rew, done, info = env.step(a[k][off:off + n])
        out = env.get_state().clone(), obs["observation"].clone(), rew.clone(), done.clone()
        env.close()
        return out
    full = run(E, 0)
    again = run(E, 0)
    for x, y in zip(full, again):
        assert torch.equal(x, y)                                   # deterministic, bitwise
    half = run(E // 2, E // 2)
    for x, y in zip(full, half):
        assert torch.equal(x[E // 2:], y)                          # world-size invariant, bitwise
    st = full[0]
    assert torch.isfinite(st).all()
    qn = st[:, 21:25].norm(dim=1)
    assert (qn - 1).abs().max() < 1e-5
    assert (st[:, 7:9] > -5e-3).all() and (st[:, 7:9] < 0.045).all()      # limit rows are soft (ERP 0.2)
    assert ((full[2] == 0) | (full[2] == 1)).all()
    assert (st[:, 52] == 3).all() | (full[3] != 0).any()


def test_full_size_properties_16384(gx):
    """BASELINE config 3 (16 384 envs on one GPU): same size-independent properties on the one-env-per-lane step
    kernel below the headline size (256 wavefronts), with the per-step resets on the cooperative kernel"""
    E = 16384
    a = [torch.rand(E, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(10 + k)) * 2 - 1 for k in range(4)]

    def run(n, off):
        env = gx.make("XarmPDPickAndPlace-v0", num_envs=n, seed=23, env_id_offset=off)
        env.reset()
        env.set_episode_steps((torch.arange(n, device="cuda") + off) % 50)      # time-limit resets in every call
        for k in range(4):
            obs, rew, done, info = env.step(a[k][off:off + n])
        out = env.get_state().clone(), obs["observation"].clone(), rew.clone(), done.clone()
        env.close()
        return out
    full, again = run(E, 0), run(E, 0)
    for x, y in zip(full, again):
        assert torch.equal(x, y)
    tail = run(E - 12288, 12288)          # a 4 096-env shard steps on k_step_coop: equal within float32, not bitwise
    st = full[0]
    assert torch.isfinite(st).all() and float((st[:, 21:25].norm(dim=1) - 1).abs().max()) < 1e-5
    assert bool((st[:, 34:50] >= 0).all())
    assert bool(torch.equal(st[12288:, 31:34], tail[0][:, 31:34])) and bool(torch.equal(st[12288:, 52:], tail[0][:, 52:]))   # goals, counters
    err = (st[12288:, :18] - tail[0][:, :18]).abs().max(dim=1).values
    assert float(err.median()) < 1e-4
    ep = st[:, 53]
    assert int((ep == 2).sum()) >= 4 * E // 50 - 8             # four calls x E / 50 time-limit resets (+ successes)


def test_world_size_invariance_at_the_baseline_split(gx):
    """'1-GPU vs 8-GPU bitwise-equal per env' at BASELINE's own split - 65 536 envs on one handle against the
    8 192-env shard [k 8192, (k + 1) 8192) a rank of an 8-GPU job owns.  By default the shard would step on the cooperative
    kernels and the full batch on the fast pipeline (equal to float32 rounding only); with the kernel family pinned from
    the job's config (gym_xarm_amd.distributed.reproducible_limits) the results are bitwise equal - in
    every family - and the default pin ('fast') keeps the speed of the unpinned handle."""
    import time
    from gym_xarm_amd import distributed as D
    E, n, k = 65536, 8192, 5
    off = k * n
    a = [torch.rand(E, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(40 + j)) * 2 - 1 for j in range(3)]
    assert D.reproducible_limits(E) == {"reset_coop_limit": E, "step_coop_limit": 1} == D.reproducible_limits(E, "fast")
    assert D.reproducible_limits(E, "lane") == {"reset_coop_limit": -1, "step_coop_limit": -1}
    assert D.reproducible_limits(4096) == {"reset_coop_limit": 4096, "step_coop_limit": 4096}

    def run(num, offset, limits, timed=0):
        env = gx.make("XarmPDPickAndPlace-v0", num_envs=num, seed=29, env_id_offset=offset, **limits)
        lim, pipe = env.kernel_limits(), env.pipeline_info()
        env.reset()
        env.set_episode_steps((torch.arange(num, device="cuda") + offset) * 7919 % 50)    # time-limit resets in every call
        for j in range(3):
            obs, rew, done, info = env.step(a[j][offset:offset + num])
        out = env.get_state().clone(), obs["observation"].clone(), rew.clone(), done.clone()
        rate = None
        if timed:
            for j in range(10):
                env.step(a[j % 3][offset:offset + num])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for j in range(timed):
                env.step(a[j % 3][offset:offset + num])
            torch.cuda.synchronize()
            rate = num * timed / (time.perf_counter() - t0)
        env.close()
        return out, lim, pipe, rate
    rates = {}
    for family in ("fast", "lane", "coop"):
        limits = D.reproducible_limits(E, family)
        full, lim_full, pipe_full, rates[family] = run(E, 0, limits, timed=60 if family == "fast" else 0)
        shard, lim_shard, pipe_shard, _ = run(n, off, limits)
        assert lim_full == lim_shard == {"fast": (E, 1), "lane": (0, 0), "coop": (E, E)}[family]
        assert pipe_full == pipe_shard and pipe_full["fast_pipeline"] == (family == "fast")
        if family == "fast":
            assert pipe_full["eject_coop_cap"] == 2 ** 31 - 1            # the hand-off kernel is not chosen by a count
        for x, y in zip(full, shard):
            assert torch.equal(x[off:off + n], y), family                      # bitwise, per env
        assert int((full[0][:, 53] >= 2).sum()) >= 3 * E // 50 - 8             # resets really ran inside the step calls
    # the default (per-shard) choice: same envs, different kernel family -> float32-close, not bitwise
    dflt, lim, pipe, _ = run(n, off, {})
    assert lim == (8192, 8192) and not pipe["fast_pipeline"]
    err = (dflt[0][:, :18] - full[0][off:off + n, :18]).abs().max(dim=1).values
    assert float(err.median()) < 1e-4 and bool(torch.equal(dflt[0][:, 31:34], full[0][off:off + n, 31:34]))
    # the pinned 65 536-env handle keeps the speed of the default one (within 10 %)
    _, _, pipe_d, rate_default = run(E, 0, {}, timed=60)
    assert pipe_d["fast_pipeline"] and rates["fast"] > 0.9 * rate_default, (rates["fast"], rate_default)
    print("env steps/s at 65 536 envs: default %.3g, reproducible 'fast' pin %.3g" % (rate_default, rates["fast"]))


@pytest.mark.parametrize("env_id,E,A", [("XarmPDPickAndPlace-v0", 16384, 4), ("XarmReach-v0", 512, 4), ("XarmPDStackTower-v0", 512, 8),
                                        ("XarmPDHandover-v0", 4096, 8), ("XarmPDHandover-v0", 512, 8)])   # Handover: the fast pipeline / the cooperative step
def test_a_captured_step_replays_like_eager_steps(gx, env_id, E, A):
    """xarm_step keeps no host-side per-step state (its device counters are zeroed by a memset inside the call), forks and
    joins its side stream inside the call: one step captured into a HIP graph (torch.cuda.graph) and replayed with new
    actions gives the bits of eager steps - incl. the auto-resets, the hand-off lists and StackTower's class order"""
    def run(capture):
        env = gx.make(env_id, num_envs=E, seed=1)
        env.reset()
        env.set_episode_steps(torch.arange(E, device=env.device) % env._max_episode_steps)
        gen = torch.Generator(device="cuda").manual_seed(0)
        acts = [torch.rand(E, A, device="cuda", generator=gen) * 2 - 1 for _ in range(6)]
        a = acts[0].clone()
        outs = []
        if capture:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                env.step(a)                       # first call outside the capture
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                obs, rew, done, info = env.step(a)
            for k in range(1, 6):
                a.copy_(acts[k])
                graph.replay()
                outs.append(torch.cat([obs["observation"], rew[:, None], done[:, None].float(), env.get_state()], 1).clone())
        else:
            env.step(a)
            for k in range(1, 6):
                obs, rew, done, info = env.step(acts[k])
                outs.append(torch.cat([obs["observation"], rew[:, None], done[:, None].float(), env.get_state()], 1).clone())
        torch.cuda.synchronize()
        env.close()
        return torch.stack(outs)
    eager, replay = run(False), run(True)
    assert torch.isfinite(eager).all() and torch.equal(eager, replay)


def test_overlapped_reset_changes_nothing_but_the_time(gx, monkeypatch):
    """A pipelined PickAndPlace step resets the episodes that ended in k_step_fast_stage on a side stream while the hand-off still
    runs, and those that ended in the hand-off after it (two lists, two launches, joined before the call's work ends on the
    caller's stream).  XARM_RESET_OVERLAP=0 runs both resets on the caller's stream: same bits, through several hundred
    resets per step."""
    E = 20000

    def run():
        env = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=13, step_coop_limit=1)
        env.reset()
        env.set_episode_steps(torch.arange(E, device=env.device) % 50)
        gen = torch.Generator(device="cuda").manual_seed(3)
        rec = []
        for _ in range(6):
            obs, rew, done, info = env.step(torch.rand(E, 4, device="cuda", generator=gen) * 2 - 1)
            rec.append(torch.cat([obs["observation"], obs["achieved_goal"], obs["desired_goal"], rew[:, None], done[:, None].float(),
                                  info["terminal_observation"], env.get_state()], dim=1).clone())
        env.close()
        return torch.stack(rec)
    on = run()
    monkeypatch.setenv("XARM_RESET_OVERLAP", "0")
    off = run()
    assert torch.isfinite(on).all() and torch.equal(on, off)
    assert int(on[:, :, 32].sum()) > 6 * 300          # done flags: the resets were really exercised


def test_staged_pipeline_against_the_unstaged_one(gx, monkeypatch):
    """The pipelined PickAndPlace step runs its fast kernel in three stages of five substeps (XARM_PNP_STAGES_DEFAULT), each stage's hand-off
    re-running the substeps from that stage's first one on the cooperative kernel beside the next stage - against XARM_PNP_STAGES=1 (one fast
    launch, one hand-off: the single stage {0, 15} of the same kernels) from identical states: an env that finishes on the fast path or is handed off in the first
    stage runs the same code over the same substeps - the same bits; an env whose pads come alive later has its first substeps on the
    lane core instead of the cooperative one - float32-close.  Run to run the staged step is bitwise reproducible (three streams), with
    auto-reset as without."""
    E = 16384
    staged = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=41, auto_reset=False)
    monkeypatch.setenv("XARM_PNP_STAGES", "1")
    plain = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=41, auto_reset=False)
    monkeypatch.delenv("XARM_PNP_STAGES")
    assert staged.stage_info() == [0, 5, 10, 15] and plain.stage_info() == [0, 15]
    staged.reset()
    gen = torch.Generator(device="cuda").manual_seed(77)
    n_same = n_late = n_handed = 0
    for t in range(12):
        a = torch.rand(E, 4, device="cuda", generator=gen) * 2 - 1
        st0 = staged.get_state().clone()
        plain.set_state(st0)
        obs, rew, done, _ = staged.step(a)
        ref, handed = staged.get_state().clone(), staged.debug_counts()[1]
        pobs, prew, pdone, _ = plain.step(a)
        assert abs(plain.debug_counts()[1] - handed) <= 0.02 * handed + 2          # the same envs are handed off (but for borderline pads)
        same = (ref == plain.get_state()).all(dim=1)
        d = (ref - plain.get_state())[:, :31].abs().max(dim=1).values
        assert float((d < 1e-3).float().mean()) > 0.995, (t, float(d.max()), float((d < 1e-3).float().mean()))
        assert torch.equal(rew[same], prew[same]) and torch.equal(done[same], pdone[same]) and torch.equal(obs["observation"][same], pobs["observation"][same])
        n_same += int(same.sum()); n_late += int((~same).sum()); n_handed += handed
        staged.set_state(st0)
        staged.step(a)
        assert torch.equal(staged.get_state(), ref)                                  # run to run
    assert n_handed > 12 * E // 100 and 0 < n_late < n_handed and n_same > 0.97 * 12 * E, (n_same, n_late, n_handed)
    staged.close()
    plain.close()
    env = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=42)                      # auto-reset: two runs, the same bits
    outs = []
    env.reset()
    s0 = env.get_state().clone()
    s0[:, 52] = (torch.arange(E, device="cuda") * 7919 % 50).float()                 # episode phases spread: ~330 resets per call
    for rep in range(2):
        env.set_state(s0)
        g2 = torch.Generator(device="cuda").manual_seed(5)
        for t in range(6):
            env.step(torch.rand(E, 4, device="cuda", generator=g2) * 2 - 1)
        outs.append(env.get_state().clone())
    assert torch.equal(outs[0], outs[1])
    env.close()


def test_fast_pipeline_against_the_plain_step_kernel(gx, monkeypatch):
    """What a large PickAndPlace batch steps on by default - k_step_fast_stage (the pad-free substep) with the hand-off of the
    envs that have an active finger-pad row to k_step_coop_list_stage - against the plain k_step.  The fast substep is the plain
    one minus blocks that are no-ops for an env without pad rows: the same bits in the host build (tests/test_hostcore.py)
    and in a device build with -ffp-contract=on (measured: 71 of 4 096 envs differ after a step, the handed-off ones); the
    default device build lets LLVM contract the two instantiations differently, so here an env that is never handed off
    agrees to float32 rounding (last bits of the joint velocities), a handed-off env likewise (cooperative core) until
    contact chaos separates the trajectories.  XARM_STEP_PIPELINE=0 and step_coop_limit < 0 select the plain kernel."""
    E = 8192
    a = [torch.rand(E, 4, device="cuda", generator=torch.Generator(device="cuda").manual_seed(70 + j)) * 2 - 1 for j in range(4)]

    def run(**kw):
        env = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=31, auto_reset=False, reset_coop_limit=-1, **kw)
        o = env.reset()["observation"]
        sts, dist = [], [(o[:, 0:3] - o[:, 8:11]).norm(dim=1).clone()]       # hand COM to object centre
        for j in range(4):
            o = env.step(a[j])[0]["observation"]
            sts.append(env.get_state().clone())
            dist.append((o[:, 0:3] - o[:, 8:11]).norm(dim=1).clone())
        env.close()
        return sts, dist
    (fast, _), (plain, dist) = run(step_coop_limit=1), run(step_coop_limit=-1)
    far = torch.ones(E, dtype=torch.bool, device="cuda")
    for j in range(4):
        # the hand COM travels < 7 cm per step, the pad spheres sit < 9 cm from it and the object's corners < 5.3 cm from its
        # centre: an env whose object centre was more than 22 cm from the hand COM before and after every step so far kept
        # > 4 cm between pads and object, far outside the 5 mm solver margin - it was never handed off
        far &= (dist[j] > 0.22) & (dist[j + 1] > 0.22)
        err = (fast[j][:, :31] - plain[j][:, :31]).abs().max(dim=1).values
        assert float(err[far].max()) < 2e-4 * (j + 1), (j, float(err[far].max()))   # never handed off: rounding only, no chaos
        assert float(err.median()) < 1e-5, j
        assert bool(torch.equal(fast[j][:, 31:34], plain[j][:, 31:34])) and bool(torch.equal(fast[j][:, 52:], plain[j][:, 52:]))   # goals, counters
        touch_f, touch_p = fast[j][:, 50], plain[j][:, 50]
        assert float((touch_f != touch_p).float().mean()) < 0.01             # the contact flags agree but for borderline envs
    assert int(far.sum()) > 200
    monkeypatch.setenv("XARM_STEP_PIPELINE", "0")
    off, _ = run(step_coop_limit=1)
    for x, y in zip(off, plain):
        assert torch.equal(x, y)                                                      # the override selects the plain kernel


def test_env_override_applies_to_the_default_limits_only(gx, monkeypatch):
    """XARM_RESET_COOP_LIMIT / XARM_STEP_COOP_LIMIT replace the built-in DEFAULT; an explicit xarm_config value - incl.
    '< 0 = never' - wins (include/xarm_hip.h xarm_kernel_limits)"""
    monkeypatch.setenv("XARM_RESET_COOP_LIMIT", "1024")
    monkeypatch.setenv("XARM_STEP_COOP_LIMIT", "2048")
    for kw, want in (({}, (1024, 2048)), ({"reset_coop_limit": -1, "step_coop_limit": -1}, (0, 0)),
                     ({"reset_coop_limit": 512, "step_coop_limit": 256}, (512, 256))):
        env = gx.make("XarmPDPickAndPlace-v0", num_envs=64, seed=1, **kw)
        assert env.kernel_limits() == want, (kw, env.kernel_limits())
        env.close()


def test_dense_reward_on_grasp_rollout(gxk, oracle, golden_rollout, parity):
    """reward_type='dense' (:166-175): staged reward incl. the contact-flag branches, HIP vs oracle"""
    g = golden_rollout
    S, A = g["grasp_states"], g["grasp_actions"]
    E = S.shape[1]
    env = gxk.make("XarmPDPickAndPlace-v0", num_envs=E, seed=1, auto_reset=False,
                  config=dict(gxk.vec_env.CONFIG_DEFAULTS, reward_type="dense"))
    ora = oracle.OraclePnP(E, seed=1, reward_type="dense")
    seen = set()
    for t in range(A.shape[0]):
        env.set_state(S[t])
        ora.set_state(S[t])
        obs, rew, done, info = env.step(torch.tensor(A[t], dtype=torch.float32))
        o = ora.step(A[t])
        ok = (g["grasp_sens"][t] < 1e-3) & (_np(env.get_state())[:, 50] == ora.state[:, 50])
        np.testing.assert_allclose(_np(rew)[ok], o[3][ok], atol=2e-4)
        seen |= set(np.round(o[3][ok], 1))
    assert 0.5 in seen and any(r > 1.0 for r in seen) and any(r < 0.3 for r in seen)   # all three stages occurred
    with pytest.raises(Exception, match="relabel"):
        env.compute_reward(torch.zeros(2, 3), torch.zeros(2, 3))
    env.close()


def test_run_demo_literal_replay(gx, oracle):
    """XarmPickAndPlace._run_demo (xarm_pick_and_place.py:310-349) replayed tick by tick through the C ABI
    (xarm_debug_substeps / get_state / set_state) next to the oracle's replay: same grasp, same lift"""
    E = 16
    ora = oracle.OraclePnP(E, seed=4)
    ora.reset()
    So = oracle.run_demo(ora, ora.get_state, ora.set_state, ora.debug_substeps)
    env = gx.make("XarmPDPickAndPlace-v0", num_envs=E, seed=4, auto_reset=False)
    env.reset()
    Sd = oracle.run_demo(env, lambda: _np(env.get_state()), lambda s: env.set_state(torch.tensor(s, dtype=torch.float32)),
                         lambda qt, n: env.debug_substeps(torch.tensor(qt, dtype=torch.float32), n))
    assert (Sd[-1, :, 20] > 0.2).all() and (Sd[-1, :, 50] == 1).all() and (Sd[10:13, :, 50] == 1).all()
    np.testing.assert_allclose(Sd[-1, :, 18:21], So[-1, :, 18:21], atol=5e-3)       # 23 free-running ticks, float32 vs float64
    np.testing.assert_allclose(Sd[-1, :, :7], So[-1, :, :7], atol=5e-3)
    env.close()


def test_auto_reset_matches_oracle_step_then_reset(gxk, oracle):
    """auto-reset path (k_step -> done list -> k_reset) against oracle.step followed by oracle.reset(mask)"""
    E = 128
    env = gxk.make("XarmPDPickAndPlace-v0", num_envs=E, seed=31, config=dict(gxk.vec_env.CONFIG_DEFAULTS, goal_shape="ground"))
    ora = oracle.OraclePnP(E, seed=31, goal_shape="ground")
    env.reset()
    for _ in range(12):                       # let the objects settle, arm at rest
        env.step(torch.zeros(E, 4))
    st = _np(env.get_state()).astype(np.float64)
    st[::2, 52] = 49
    env.set_state(st)
    ora.set_state(st)
    a = torch.zeros(E, 4)
    a[:, 2] = 0.5
    obs, rew, done, info = env.step(a)
    o_obs, o_ag, o_dg, o_rew, o_done, o_succ = ora.step(a.numpy().astype(np.float64))
    assert np.array_equal(_np(done), o_done) and o_done[::2].all()
    term = _np(info["terminal_observation"])
    calm = np.abs(st[:, 19]) > 0.09           # object away from the fingers: well-conditioned envs
    np.testing.assert_allclose(term[o_done.astype(bool) & calm], o_obs[o_done.astype(bool) & calm], atol=2e-3)
    ora.reset(mask=o_done)
    dev = _np(env.get_state()).astype(np.float64)
    ok = calm & (np.abs(ora.state[:, 19]) > 0.09)
    np.testing.assert_allclose(dev[ok, :31], ora.state[ok, :31], atol=4e-3)
    np.testing.assert_allclose(dev[:, 31:34], ora.state[:, 31:34], atol=1e-6)          # goals: same counter RNG
    assert (dev[:, 33] == np.float32(0.025)).all()                                      # goal_shape='ground'
    assert np.array_equal(dev[:, 52:54], ora.state[:, 52:54])
    env.close()


def test_scripted_pick_and_lift_rate(gxk, tmp_path):
    """behavioural regression (cf. the reference's _run_demo :310-349): the closed-loop scripted policy lifts
    most objects that do not start under the gripper; also snapshot / restore of the simulator state"""
    from gym_xarm_amd.policies import lift_stages
    E = 2048
    env = gxk.make("XarmPDPickAndPlace-v0", num_envs=E, seed=5, auto_reset=False)
    st = lift_stages(env)
    # oracle, 192 envs: hovered 0.92, contact 0.94, raised 0.91, lifted 0.91 (tests/test_policies.py); objects spawned under
    # the gripper are batted off the table by the reset's own arm motion
    assert st["hovered"] > 0.8 and st["contact"] > 0.8 and st["lifted"] > 0.8 and st["lifted"] > 0.93 * st["contact"], st
    snap = str(tmp_path / "state.safetensors")
    env.save_state(snap)
    before = env.get_state().clone()
    obs1 = env.step(torch.zeros(E, 4))[0]["observation"].clone()
    env.load_state(snap)
    assert torch.equal(env.get_state(), before)
    obs2 = env.step(torch.zeros(E, 4))[0]["observation"]
    assert torch.equal(obs1, obs2)                       # restored state reproduces the step bitwise
    env.close()


def test_rollout_statistics_match_oracle(gxk, oracle):
    """Past contact onset trajectories diverge (chaotic contact dynamics), so long-horizon parity is asserted on
    distributions (SURVEY.md 7 'Hard parts'): 2048 envs x 30 random steps from the same seeds, HIP vs oracle."""
    from concurrent.futures import ThreadPoolExecutor
    E, T, W = 2048, 30, 16
    env = gxk.make("XarmPDPickAndPlace-v0", num_envs=E, seed=123, auto_reset=False)
    env.reset()
    acts = [torch.rand(E, 4, generator=torch.Generator().manual_seed(100 + t)) * 2 - 1 for t in range(T)]
    for t in range(T):
        obs, rew, done, info = env.step(acts[t])
    dev = _np(env.get_state()).astype(np.float64)
    env.close()
    shards = [oracle.OraclePnP(E // W, seed=123, env_id_offset=k * (E // W)) for k in range(W)]
    a_np = [a.numpy().astype(np.float64) for a in acts]

    def run(k):
        s = shards[k]
        s.reset()
        for t in range(T):
            s.step(a_np[t][k * (E // W):(k + 1) * (E // W)])
        return s.state
    with ThreadPoolExecutor(W) as ex:
        ora = np.concatenate(list(ex.map(run, range(W))))

    def stats(s):
        on_table = (s[:, 20] > 0.02) & (s[:, 20] < 0.1)
        return np.array([on_table.mean(), (s[:, 20] < -0.05).mean(), (s[:, 20] > 0.1).mean(), s[:, 50].mean(),
                         np.median(s[:, 18]), np.median(np.abs(s[:, 19])), s[:, 7].mean(), np.abs(s[:, 9:16]).mean()])
    sd, so = stats(dev), stats(ora)
    # fractions agree within 3 sigma of a binomial with n = 2048 (<= 0.035) plus model noise; medians within 1 cm
    tol = np.array([0.04, 0.04, 0.04, 0.04, 0.01, 0.01, 0.002, 0.05])
    assert (np.abs(sd - so) <= tol).all(), (sd, so)
    # the arm itself is well conditioned: joint angles of envs whose object never came near the gripper agree closely
    calm = (np.abs(ora[:, 20] - 0.04) < 1e-3) & (np.abs(dev[:, 20] - 0.04) < 1e-3) & (ora[:, 50] == 0)
    assert calm.mean() > 0.2
    assert np.median(np.abs(dev[calm, :7] - ora[calm, :7]).max(axis=1)) < 2e-3


def test_contact_regime_256_envs(gxk, oracle, parity):
    """The grasp / contact regime with a fixture that bites: 256 envs under the scripted reach-grasp-lift with per-env
    jitter (tests/tools/gen_oracle_fixtures.JitteredGrasp), every transition replayed on the device from the oracle's
    state.  Thresholds are what the kernels achieve, not what they are allowed: >= 90 % of the envs inside the plain
    5e-4 + 2e-4|x| bound at EVERY step, <= 10 % exempt (sens > 0.05), the allowance of the rest capped at 1e-2, and the
    rows that are in contact (pad impulses / touch flag) held to the same numbers separately."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    from gen_oracle_fixtures import JitteredGrasp
    E = 256
    ora = oracle.OraclePnP(E, seed=61)
    ora.reset()
    for _ in range(3):
        ora.step(np.zeros((E, 4)))
    env = gxk.make("XarmPDPickAndPlace-v0", num_envs=E, seed=61, auto_reset=False)
    pol = JitteredGrasp(E, seed=5)
    worst_tight, worst_exempt, n_contact, n_contact_tight, n_flag, n_ok = 1.0, 0.0, 0, 0, 0, 0
    for t in range(pol.horizon):
        st0 = ora.get_state()
        a = pol(st0, t)
        nxt, o_obs, o_ag, o_dg, o_rew, o_done, o_succ, sens = parity.oracle_step_with_sens(ora, st0, a, seed=t)
        env.set_state(st0)
        obs, rew, done, info = env.step(torch.tensor(a, dtype=torch.float32))
        dev = _np(env.get_state()).astype(np.float64)
        stats = parity.compare(dev[:, parity.CONT], nxt[:, parity.CONT], sens, what="contact regime t=%d" % t, frac_tight=0.9, max_exempt=0.1)
        worst_tight, worst_exempt = min(worst_tight, stats["frac_tight"]), max(worst_exempt, stats["frac_exempt"])
        contact = ((np.abs(nxt[:, 42:50]) > 0).any(axis=1) | (nxt[:, 50] > 0)) & (sens <= parity.SENS_EXEMPT)
        err = np.abs(dev[:, parity.CONT] - nxt[:, parity.CONT])
        tight = (err <= parity.ATOL + parity.RTOL * np.abs(nxt[:, parity.CONT])).all(axis=1)
        n_contact += contact.sum()
        n_contact_tight += (contact & tight).sum()
        ok = sens < 1e-3
        assert np.array_equal(_np(rew)[ok], o_rew[ok].astype(np.float32)) and np.array_equal(_np(done)[ok], o_done[ok])
        n_flag += (dev[ok, 50] == nxt[ok, 50]).sum()
        n_ok += ok.sum()
        assert (dev[:, 34:50] >= 0).all()                       # normal impulses never pull
    lifted = nxt[:, 20] > 0.15
    print("contact regime (%s): worst frac_tight %.3f, worst frac_exempt %.3f, contact rows %d (%.3f tight), lifted %.2f"
          % (gxk.family, worst_tight, worst_exempt, n_contact, n_contact_tight / max(n_contact, 1), lifted.mean()))
    assert n_contact > 1500 and n_contact_tight >= 0.9 * n_contact
    assert n_flag >= 0.98 * n_ok
    assert lifted.mean() > 0.4                                   # the script really grasps and lifts in the oracle
    # free-running device rollout under the same closed-loop script: invariants of the contact phase + the lift rate
    env.reset()
    for _ in range(3):
        env.step(torch.zeros(E, 4))
    pol = JitteredGrasp(E, seed=5)
    for t in range(pol.horizon):
        st = _np(env.get_state()).astype(np.float64)
        env.step(torch.tensor(pol(st, t), dtype=torch.float32))
        s = _np(env.get_state())
        assert np.isfinite(s).all() and (s[:, 34:50] >= 0).all()
        on_table = (np.abs(s[:, 18]) < 0.7) & (np.abs(s[:, 19]) < 0.45)
        assert (s[on_table, 20] > 0.02).all()                    # never pressed into the table (half extents 0.025 / 0.04)
        assert (np.abs(np.linalg.norm(s[:, 21:25], axis=1) - 1) < 1e-5).all()
    dev_lifted = s[:, 20] > 0.15
    held = dev_lifted & (s[:, 50] > 0)
    assert abs(dev_lifted.mean() - lifted.mean()) < 0.08, (dev_lifted.mean(), lifted.mean())
    assert held.sum() >= 0.9 * dev_lifted.sum()                  # lifted means held between the pads
    env.close()
