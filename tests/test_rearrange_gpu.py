"""XarmRearrange-v0 on the GPU, through the C ABI and the VecEnv: registry and call surface, the device against StackTower's
oracle with a parked cube, against the host float64 core on four-cube contact states, the reward kernel, the class order,
the BASELINE-sized batch, a scripted episode, rendering and HER relabelling.
Held to the host float64 core beyond the state after a step: k_ra_init and the draw keying across the 2^32 env-id boundary, the
full and the masked device reset (against rearrange_host.reset_reference: the reset spelled out around one bare tick), every
step output (obs, ag, dg, reward, done, is_success), the step's reward against compute_reward, and auto-resetting calls
(terminal observation, post-reset outputs, new goals) with the class order on and off."""
import os

import numpy as np
import pytest

import rearrange_host as R
from test_rearrange_host import POS, RESET_E, RESET_SEED, reset_batch_actions

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
S_CONT = np.r_[0:36, 54:93]          # StackTower: q, qd of both arms, cube poses and velocities
PARK = {0: (0.0, 0.45), 1: (0.0, -0.45), 2: (0.0, 0.45), 3: (0.0, -0.45)}
pytestmark = pytest.mark.gpu


def _make(E, **kw):
    import gym_xarm_amd
    return gym_xarm_amd.make("XarmRearrange-v0", num_envs=E, **kw)


def _perturb3(s, rng, eps=1e-6):
    s = np.array(s, dtype=np.float64, copy=True)
    s[:, S_CONT] += rng.uniform(-eps, eps, size=(s.shape[0], S_CONT.size))
    for o in range(3):
        q = s[:, 63 + 4 * o:67 + 4 * o]
        s[:, 63 + 4 * o:67 + 4 * o] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return s


def _np(t):
    return t.cpu().numpy()


def _np64(t):
    return t.cpu().numpy().astype(np.float64)


def _goal_distance(ag, dg):
    return np.linalg.norm(np.asarray(ag, dtype=np.float64) - np.asarray(dg, dtype=np.float64), axis=1)


def _stack_obs(o, parked):
    """the StackTower view [E, 55] of Rearrange observations [E, 68] (cube blocks through live_cubes, as the CPU test _run_parked):
    positions 3, quaternions 4, linear and angular velocities 3 per live cube, then both arms"""
    out = np.zeros((o.shape[0], 55))
    for p in range(4):
        m = parked == p
        for j, c in enumerate(R.live_cubes(p)):
            out[m, 3 * j:3 * j + 3] = o[m, 3 * c:3 * c + 3]
            out[m, 9 + 4 * j:13 + 4 * j] = o[m, 12 + 4 * c:16 + 4 * c]
            out[m, 21 + 3 * j:24 + 3 * j] = o[m, 28 + 3 * c:31 + 3 * c]
            out[m, 30 + 3 * j:33 + 3 * j] = o[m, 40 + 3 * c:43 + 3 * c]
    out[:, 39:55] = o[:, 52:68]
    return out


def _check_step_outputs(parity, obs, rew, done, info, dev_state, h_obs, h_done, h_dist, sens, what, to_ref=lambda o: o):
    """the outputs of one device step against the host's: obs through parity.compare (to_ref maps the device observation onto the
    reference's layout), ag / dg bit-equal to their sources, done, and reward / is_success away from the 0.12 shell"""
    o, ag, dg = _np(obs["observation"]), _np(obs["achieved_goal"]), _np(obs["desired_goal"])
    stats = parity.compare(to_ref(o.astype(np.float64)), h_obs, sens, frac_tight=0.7, max_exempt=0.15, what=what + " obs")
    assert np.array_equal(ag, o[:, 0:12]) and np.array_equal(dg, dev_state[:, R.GOAL:R.GOAL + 12])
    assert np.array_equal(_np(done), h_done)
    clear = np.abs(h_dist - 0.12) > 1e-4
    assert np.array_equal(_np(rew)[clear], np.where(h_dist > 0.12, -1.0, 0.0).astype(np.float32)[clear])
    assert np.array_equal(_np(info["is_success"])[clear], (h_dist < 0.12).astype(np.uint8)[clear])
    return stats


def _check_reset(parity, dev_state, out, ref, sens, rows, what):
    """device state and outputs after a reset against reset_reference's on `rows`; -> the worst non-exempt error per block"""
    o, ag = _np64(out["observation"])[rows], _np64(out["achieved_goal"])[rows]
    st, sens = dev_state[rows], sens[rows]
    kw = dict(frac_tight=0.7, max_exempt=0.15)
    worst = {}
    for name, x, y in (("pos", st[:, POS], ref[0][rows][:, POS]), ("vel", st[:, R.BV:R.BV + 24], ref[0][rows][:, R.BV:R.BV + 24]),
                       ("obs", o, ref[1][rows]), ("ag", ag, ref[2][rows])):
        worst[name] = parity.compare(x, y, sens, what="%s %s" % (what, name), **kw)["max_err"]
    return worst


def test_gpu_rearrange_make_dims_registry_and_shell():
    import torch
    import ctypes as C
    import gym_xarm_amd
    from gym_xarm_amd import _native
    from gym_xarm_amd.envs import XarmRearrangeEnv, XarmPDBimanualEnv
    for i in ("XarmRearrange-v0", "XarmPDRearrange-v0", "XarmPDBimanual-v0"):
        assert gym_xarm_amd.spec(i)["max_episode_steps"] == 50
    env = _make(64, seed=1)
    assert (env.obs_dim, env.goal_dim, env.act_dim, env.state_dim, env.max_episode_steps) == (68, 12, 8, 160, 50)
    assert env.action_space.shape == (8,) and env.observation_space["observation"].shape == (68,)
    assert env.observation_space["desired_goal"].shape == (12,) and env.distance_threshold == pytest.approx(0.12)
    obs = env.reset()
    assert torch.equal(obs["observation"][:, 0:12], obs["achieved_goal"])
    assert bool((obs["desired_goal"].reshape(64, 4, 3)[..., 2] == 0.025).all())
    obs, rew, done, info = env.step(torch.zeros(64, 8, device=env.device))
    assert "TimeLimit.truncated" in info and not bool(done.any())
    assert env.class_keys().shape == (64,)
    env.close()
    with pytest.raises(NotImplementedError):
        _make(4, config={"num_obj": 3})
    with pytest.raises(NotImplementedError):
        _make(4, config={"reward_type": "dense_o2g"})
    # the ABI itself refuses what StackTower refuses
    L = _native.load()
    for num_obj, rt, stand, ar in ((3, 0, 0, 0), (4, 2, 0, 0), (4, 0, 1, 0), (4, 0, 0, 2)):
        cfg = _native.XarmConfig(8, 0, 0, _native.ENV_REARRANGE, num_obj, rt, 0, 0.0, 0.0, ar, 0, 0.0, 0, 0, stand)
        h = C.c_void_p(0)
        assert L.xarm_create(C.byref(cfg), C.byref(h)) != 0
        assert L.xarm_last_error(None)
    # the single-env shell: the reference's call surface
    e = XarmRearrangeEnv()
    assert XarmPDBimanualEnv is XarmRearrangeEnv and e.num_obj == 4 and e._max_episode_steps == 50
    o = e.reset()
    assert o["observation"].shape == (68,) and o["desired_goal"].shape == (12,)
    o, r, d, inf = e.step(np.zeros(8))
    assert d is False and r in (-1.0, 0.0) and "is_success" in inf
    assert e.compute_reward(o["achieved_goal"], o["desired_goal"], {}) == r
    with pytest.raises(AssertionError):
        e.step(np.zeros(4))
    assert e.render(width=32, height=24).shape == (24, 32, 4)
    e.close()


def test_gpu_rearrange_parked_cube_against_oracle(oracle, parity):
    """256 envs x 6 steps: a StackTower state per env with cube (env % 4) parked; the device must follow OracleStackTower"""
    import torch
    E = 256
    ora = oracle.OracleStackTower(E, seed=6)
    ora.reset()
    s3 = ora.get_state()
    s3[0:32, 57:60] = s3[0:32, 54:57] + [0.03, 0.004, 0.0]             # overlapping cubes
    s3[32:64, 57:60] = s3[32:64, 54:57] + [0.002, -0.001, 0.05]         # towers
    s3[32:64, 60:63] = s3[32:64, 54:57] + [0.0, 0.002, 0.10]
    parked = np.arange(E) % 4
    rows = np.zeros((E, 160))
    for p in range(4):
        m = parked == p
        rows[m] = R.from_stack(s3[m], p, PARK[p])
    env = _make(E, seed=6, auto_reset=False)
    env.set_state(torch.tensor(rows, dtype=torch.float32, device=env.device))
    park0 = np.array([rows[e, R.BP + 3 * parked[e]:R.BP + 3 * parked[e] + 3] for e in range(E)])
    rng = np.random.default_rng(2)
    worst = None
    for k in range(6):
        dev0 = env.get_state().cpu().numpy().astype(np.float64)
        st = np.zeros_like(s3)
        for p in range(4):
            m = parked == p
            st[m] = R.to_stack(dev0[m], p, s3[m])
        act = rng.uniform(-1, 1, (E, 8)).astype(np.float32)
        act[:, 2] -= 0.3; act[:, 6] -= 0.3
        act = np.clip(act, -1, 1)
        ora.set_state(st)
        o_obs, o_ag, o_dg, _, o_done, _ = ora.step(act.astype(np.float64))
        nxt = ora.get_state()
        sens = np.zeros(E)
        sens_o = np.zeros(E)
        for j in range(2):
            ora.set_state(_perturb3(st, np.random.default_rng(100 * k + j)))
            p_obs = ora.step(act.astype(np.float64))[0]
            sens = np.maximum(sens, np.abs(ora.get_state()[:, S_CONT] - nxt[:, S_CONT]).max(axis=1))
            sens_o = np.maximum(sens_o, np.abs(p_obs - o_obs).max(axis=1))
        obs, rew, done, info = env.step(torch.from_numpy(act).to(env.device))
        # the outputs: the oracle's observation is StackTower's (three cubes); its goal distance is Rearrange's up to the parked
        # cube's drift (< 1e-3 m, below: < 5e-6 at the 0.12 shell), the threshold is Rearrange's
        _check_step_outputs(parity, obs, rew, done, info, env.get_state().cpu().numpy(), o_obs, o_done, _goal_distance(o_ag, o_dg),
                                      np.maximum(sens, sens_o), "Rearrange parked step %d" % k, to_ref=lambda o: _stack_obs(o, parked))
        dev = env.get_state().cpu().numpy().astype(np.float64)
        mine = np.zeros_like(nxt)
        for p in range(4):
            m = parked == p
            mine[m] = R.to_stack(dev[m], p, nxt[m])
        worst = parity.compare(mine[:, S_CONT], nxt[:, S_CONT], sens, frac_tight=0.7, max_exempt=0.15, what="Rearrange parked step %d" % k)
        s3 = nxt
    assert worst["frac_tight"] >= 0.7
    dev = env.get_state().cpu().numpy()
    drift = np.array([np.abs(dev[e, R.BP + 3 * parked[e]:R.BP + 3 * parked[e] + 3] - park0[e]).max() for e in range(E)])
    assert drift.max() < 1e-3
    env.close()


def test_gpu_rearrange_four_cube_contact_against_host(parity):
    """the device against the host float64 core on genuine four-cube contact states (blocks, towers) under random actions"""
    import torch
    from test_rearrange_host import four_cube_states, POS
    E = 48
    rows = four_cube_states(E, seed=5)
    env = _make(E, seed=5, auto_reset=False)
    env.set_state(torch.tensor(rows, dtype=torch.float32, device=env.device))
    rows = env.get_state().cpu().numpy().astype(np.float64)      # float32-rounded start for both
    rng = np.random.default_rng(9)
    many = 0
    for k in range(3):
        act = np.clip(rng.uniform(-1, 1, (E, 8)) * 0.5, -1, 1).astype(np.float32)
        nxt, obs, ag, dg, rew, done, succ, key = R.step(rows, act, f32=0, seed=5)
        many = max(many, int(sum(bin(int(x) & 0x3F).count("1") >= 3 for x in key)))
        sens = np.zeros(E)
        sens_o = np.zeros(E)
        for j in range(2):
            p = rows.copy()
            p[:, np.r_[0:36, R.BP:R.BP + 12, R.BV:R.BV + 24]] += np.random.default_rng(50 + j).uniform(-1e-6, 1e-6, (E, 72))
            ps = R.step(p, act, f32=0, seed=5)
            sens = np.maximum(sens, np.abs(ps[0][:, POS] - nxt[:, POS]).max(axis=1))
            sens_o = np.maximum(sens_o, np.abs(ps[1] - obs).max(axis=1))
        o, d_rew, d_done, d_info = env.step(torch.from_numpy(act).to(env.device))
        _check_step_outputs(parity, o, d_rew, d_done, d_info, env.get_state().cpu().numpy(), obs, done, _goal_distance(ag, dg),
                            np.maximum(sens, sens_o), "Rearrange four-cube step %d" % k)
        dev = env.get_state().cpu().numpy().astype(np.float64)
        parity.compare(dev[:, POS], nxt[:, POS], sens, frac_tight=0.7, max_exempt=0.15, what="Rearrange four-cube step %d" % k)
        rows = dev
    assert many >= E // 2, "the batch must hold envs with three or more cube pairs in contact"
    env.close()


def _goals(state):
    return np.asarray(state)[:, R.GOAL:R.GOAL + 12].reshape(-1, 4, 3)


def test_gpu_rearrange_init_matches_host_across_the_env_id_word_boundary():
    """k_ra_init against the host core's init (float32 rounding of the same affine map of the same draws: 1e-6), at env ids on
    both sides of 2^32 - the device's (uint32_t)(gid >> 32)"""
    E, big = 97, 2 ** 32
    states = {}
    for off, n in ((0, E), (big - 40, E), (big, E - 40)):
        env = _make(n, seed=11, env_id_offset=off, auto_reset=False)
        states[off] = s = _np(env.get_state())
        env.close()
        ref = R.init(n, seed=11, off=off)
        assert np.abs(s.astype(np.float64) - ref).max() <= 1e-6, off
        assert (s[:, R.STEPS] == 0).all() and (s[:, R.EPISODE] == 0).all()
        assert (_goals(s)[..., 2] == np.float32(0.025)).all() and (s[:, R.BP + 2:R.BP + 12:3] == np.float32(0.025)).all()
    assert np.array_equal(states[big], states[big - 40][40:])
    # the high word is part of the key: env 2^32 + e does not repeat env e
    assert (np.abs(_goals(states[big]) - _goals(states[0][:E - 40]))[..., :2] > 0).all()


def _stepped(E, seed, **kw):
    """a handle after the two random steps that precede the reset batches, and its float32 state as float64 rows"""
    import torch
    env = _make(E, seed=seed, **kw)
    for k in range(2):
        env.step(torch.from_numpy(reset_batch_actions(E, k)).to(env.device))
    return env, _np64(env.get_state())


def _check_goals(state, out, seed, episodes, rows=slice(None)):
    """the goals of the state and the returned desired_goal are the independent draws of `episodes` (float32 of the same map)"""
    idx = np.arange(state.shape[0])[rows]
    goal = R.drawn(seed, 0, episodes, idx)[1]
    g = _goals(state)[rows]
    assert np.abs(g[..., :2] - goal).max() <= 1e-6 and (g[..., 2] == np.float32(0.025)).all()
    assert np.array_equal(_np(out["desired_goal"])[rows], np.asarray(state, dtype=np.float32)[rows, R.GOAL:R.GOAL + 12])
    return goal


def test_gpu_rearrange_full_reset_against_reset_reference(parity):
    """k_ra_reset (no list) on 161 envs from the device's own state after two random steps, against reset_reference; then a
    second reset.  Measured on an MI355X: 18.6 % contact resets by the reference's key (30 of 161), 12.4 % exempt (20, all contact
    resets); worst non-exempt error: positions and quaternions 6.3e-5, cube velocities 3.4e-6, obs 1.2e-3 (a hand velocity), ag 3.7e-8;
    worst env in contact and not exempt 2.9e-5, worst isolated env 6.3e-5 (a joint angle)."""
    E, seed = RESET_E, RESET_SEED
    env, rows = _stepped(E, seed, auto_reset=False)
    out = env.reset()
    dev = _np(env.get_state())
    ref = R.reset_reference(rows, seed=seed)
    sens = R.reset_sens(rows, ref, seed=seed)
    contact = (ref[4] & 0x3F) != 0
    print("full reset: contact resets %.3f, exempt %.3f" % (contact.mean(), (sens > parity.SENS_EXEMPT).mean()))
    err = np.abs(dev.astype(np.float64)[:, R.RESET_FIELDS] - ref[0][:, R.RESET_FIELDS]).max(axis=1)
    print("full reset: worst env error, isolated %.2e, in contact and not exempt %.2e" % (
        err[~contact].max(initial=0), err[contact & (sens <= parity.SENS_EXEMPT)].max(initial=0)))
    worst = _check_reset(parity, dev.astype(np.float64), out, ref, sens, slice(None), "Rearrange reset")
    print("full reset: worst non-exempt error per block", worst)
    assert contact.mean() >= 0.10, "the batch must hold contact resets"
    goal1 = _check_goals(dev, out, seed, [1] * E)
    assert (dev[:, R.STEPS] == 0).all() and (dev[:, R.EPISODE] == 1).all()
    assert np.array_equal(_np(out["observation"])[:, 0:12], _np(out["achieved_goal"]))
    # cubes drawn clear of each other: no cube pair in the class key
    cube = R.drawn(seed, 0, [1] * E)[0]
    gap = np.abs(cube[:, :, None, :] - cube[:, None, :, :]).max(axis=3) + 10.0 * np.eye(4)
    clear = gap.min(axis=(1, 2)) > 0.07
    assert clear.sum() > E // 2
    assert ((_np(env.class_keys()) & 0x3F)[clear] == 0).all() and ((ref[4] & 0x3F)[clear] == 0).all()
    # episode 2
    out = env.reset()
    dev2 = _np(env.get_state())
    goal2 = _check_goals(dev2, out, seed, [2] * E)
    assert (np.abs(goal2 - goal1) > 0).all() and (dev2[:, R.EPISODE] == 2).all() and (dev2[:, R.STEPS] == 0).all()
    env.close()


def test_gpu_rearrange_masked_reset_against_reset_reference(parity):
    """k_ra_reset through the list of a ragged mask that touches both ends of two wavefronts and the last env.  Measured on an
    MI355X (none of the seven in contact, none exempt): positions 5.1e-5, cube velocities 8.6e-9, obs 8.5e-4, ag 2.4e-8."""
    import torch
    E, seed = 97, RESET_SEED
    idx = [0, 5, 31, 32, 63, 64, 96]
    m = np.zeros(E, np.uint8)
    m[idx] = 1
    env, rows = _stepped(E, seed, auto_reset=False)
    before = _np(env.get_state())
    out = env.reset(mask=torch.from_numpy(m))
    dev = _np(env.get_state())
    assert np.array_equal(dev[m == 0], before[m == 0])
    ref = R.reset_reference(rows, mask=m, seed=seed)
    sens = R.reset_sens(rows, ref, mask=m, seed=seed)
    worst = _check_reset(parity, dev.astype(np.float64), out, ref, sens, idx, "Rearrange masked reset")
    print("masked reset: worst non-exempt error per block", worst, "sens", sens[idx])
    _check_goals(dev, out, seed, [1] * len(idx), idx)
    assert (dev[idx, R.STEPS] == 0).all() and (dev[idx, R.EPISODE] == 1).all() and (dev[m == 0, R.EPISODE] == 0).all()
    assert np.array_equal(_np(out["observation"])[idx, 0:12], _np(out["achieved_goal"])[idx])
    env.close()
    # an all-ones mask is reset()
    a, _ = _stepped(E, seed, auto_reset=False)
    b, _ = _stepped(E, seed, auto_reset=False)
    oa, ob = a.reset(mask=torch.ones(E, dtype=torch.uint8)), b.reset()
    assert torch.equal(a.get_state(), b.get_state()) and torch.equal(a.class_keys(), b.class_keys())
    for k in ("observation", "achieved_goal", "desired_goal"):
        assert torch.equal(oa[k], ob[k])
    a.close(); b.close()


def test_gpu_rearrange_step_reward_is_compute_reward():
    """the reward of k_ra_step (xsqrt inside lane_step) against k_ra_compute_reward (sqrtf, another unit) of the step's own ag / dg -
    what HER relabelling assumes: sparse bit-equal off the 0.12 shell, dense within rtol 2e-6 (twelve squares summed in the same
    order and a root: contraction may move a few float32 ulps).  Measured on an MI355X: the dense gap is 0 - the two kernels gave
    the same bits in all 3 x 128 rows - and no sparse row fell within 1e-5 of the shell."""
    import torch
    E, Q4 = 128, 32
    rng = np.random.default_rng(21)
    gap = {}
    for rt in ("sparse", "dense"):
        env = _make(E, seed=8, config={"reward_type": rt})
        env.reset()
        s = _np(env.get_state())
        # half of the envs: four resting cubes clear of each other and of the arms' reach over three steps
        cube = np.zeros((2 * Q4, 4, 3), np.float32)
        cube[..., 0] = np.array([-0.2, -0.07, 0.07, 0.2], np.float32)
        cube[..., 1] = rng.uniform(-0.15, 0.15, (2 * Q4, 4))
        cube[..., 2] = 0.025
        s[:2 * Q4, R.BP:R.BP + 12] = cube.reshape(-1, 12)
        s[:2 * Q4, R.BQ:R.BQ + 16] = [0, 0, 0, 1] * 4
        s[:2 * Q4, R.BV:R.BV + 24] = 0
        s[:2 * Q4, R.LT:R.LP + 8] = 0
        # first quarter: goals on the cubes; second: at distance 0.12 -+ 1e-3 along a random direction of the 12-vector
        s[:Q4, R.GOAL:R.GOAL + 12] = s[:Q4, R.BP:R.BP + 12]
        d = rng.normal(size=(Q4, 12))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        side = np.where(np.arange(Q4) % 2 == 0, -1.0, 1.0)
        s[Q4:2 * Q4, R.GOAL:R.GOAL + 12] = s[Q4:2 * Q4, R.BP:R.BP + 12] + d * (0.12 + 1e-3 * side)[:, None]
        env.set_state(torch.from_numpy(s))
        shell = 0
        for k in range(3):
            a = torch.from_numpy(rng.uniform(-1, 1, (E, 8)).astype(np.float32) * 0.3)
            obs, rew, done, info = env.step(a)
            ag, dg, r = obs["achieved_goal"], obs["desired_goal"], _np(rew)
            again = _np(env.compute_reward(ag, dg))
            dist = _goal_distance(_np(ag), _np(dg))
            assert not bool(done.any())
            assert (dist[:Q4] < 1e-2).all() and (_np(info["is_success"])[:Q4] == 1).all()
            clear = np.abs(dist - 0.12) > 1e-5
            shell += int((~clear).sum())
            if rt == "sparse":
                assert (r[:Q4] == 0).all()
                assert np.array_equal(r[Q4:2 * Q4], np.where(side > 0, -1.0, 0.0).astype(np.float32))
                assert np.array_equal(r[clear], again[clear])
            else:
                rel = np.abs(r - again) / np.maximum(np.abs(again), 1e-30)
                rel[r == again] = 0
                gap[k] = float(rel.max())
                print("dense reward: step %d largest relative gap %.2e" % (k, gap[k]))
                assert np.allclose(r, again, rtol=2e-6, atol=0)
                assert np.allclose(r, -dist, rtol=1e-5, atol=1e-7)
        print("%s reward: %d rows within 1e-5 of the shell" % (rt, shell))
        assert shell <= 3 * E // 100
        env.close()


def _auto_reset_run(parity, flag, check):
    """four auto-resetting calls on 129 envs whose episodes end in call (env % 4); check: hold every call to step_auto.
    -> everything the calls returned, and the state after each"""
    import torch
    import gym_xarm_amd
    E, seed = 129, 12
    os.environ["XARM_RA_CLASS_ORDER"] = flag
    try:
        env = gym_xarm_amd.make("XarmRearrange-v0", num_envs=E, seed=seed, auto_reset=True)
    finally:
        del os.environ["XARM_RA_CLASS_ORDER"]
    for _ in range(6):      # the unrejected spawn of the handle's first episode settles: the envs that go on are then well conditioned,
        env.step(torch.zeros(E, 8, device=env.device))      # and the ill-conditioned transitions of a call are its resets' (and their wake)
    env.set_episode_steps(49 - torch.arange(E, device=env.device) % 4)
    who = np.arange(E) % 4
    rec, shares = [], []
    for k in range(4):
        pre = _np64(env.get_state())
        act = np.random.default_rng(40 + k).uniform(-1, 1, (E, 8)).astype(np.float32)
        obs, rew, done, info = env.step(torch.from_numpy(act).to(env.device))
        dev = _np(env.get_state())
        rec.append(torch.cat([obs["observation"], obs["achieved_goal"], obs["desired_goal"], rew[:, None], done[:, None].float(),
                              info["is_success"][:, None].float(), info["terminal_observation"] * done[:, None].float(),
                              env.get_state()], dim=1).clone())
        ended = who == k
        assert np.array_equal(_np(done) != 0, ended) and np.array_equal(_np(info["TimeLimit.truncated"]) != 0, ended)
        assert (_np(env.episode_steps())[ended] == 0).all() and np.array_equal(dev[:, R.EPISODE], pre[:, R.EPISODE] + ended)
        assert np.array_equal(dev[~ended, R.GOAL:R.GOAL + 12], pre[~ended, R.GOAL:R.GOAL + 12].astype(np.float32))
        _check_goals(dev, obs, seed, [1] * int(ended.sum()), np.where(ended)[0])
        assert np.array_equal(_np(obs["achieved_goal"]), _np(obs["observation"])[:, 0:12])
        if not check:
            continue
        ref = R.step_auto(pre, act, seed=seed)
        assert np.array_equal(ref["done"] != 0, ended)
        s = ref["step"]
        fields = np.r_[POS, R.BV:R.BV + 24]
        sens = np.zeros(E)
        for j in range(2):
            p = pre.copy()
            p[:, np.r_[0:36, R.BP:R.BP + 12, R.BV:R.BV + 24]] += np.random.default_rng(60 + 2 * k + j).uniform(-1e-6, 1e-6, (E, 72))
            ps = R.step(p, act, f32=0, seed=seed)
            sens = np.maximum(sens, np.maximum(np.abs(ps[0][:, fields] - s[0][:, fields]).max(axis=1), np.abs(ps[1] - s[1]).max(axis=1)))
        sens_step = sens.copy()
        sens[ended] = R.reset_sens(s[0], ref["reset"], mask=ended, seed=seed, rng_seed=k + 1)[ended]
        kw = dict(frac_tight=0.7, max_exempt=0.15)
        what = "Rearrange auto-reset call %d " % k
        worst = dict(
            term=parity.compare(_np64(info["terminal_observation"])[ended], ref["term"][ended], sens_step[ended], what=what + "terminal obs", **kw)["max_err"],
            obs=parity.compare(_np64(obs["observation"]), ref["obs"], sens, what=what + "obs", **kw)["max_err"],
            ag=parity.compare(_np64(obs["achieved_goal"]), ref["ag"], sens, what=what + "ag", **kw)["max_err"],
            state=parity.compare(dev.astype(np.float64)[:, fields], ref["state"][:, fields], sens, what=what + "state", **kw)["max_err"])
        assert np.abs(_np64(obs["desired_goal"]) - ref["dg"]).max() <= 1e-6
        dist = _goal_distance(s[2], s[3])
        clear = np.abs(dist - 0.12) > 1e-4
        assert np.array_equal(_np(rew)[clear], ref["rew"][clear].astype(np.float32))           # the step's reward, not the new episode's
        assert np.array_equal(_np(info["is_success"])[clear], ref["succ"][clear])
        contact = ((ref["reset"][4] & 0x3F) != 0)[ended]
        shares.append((float(contact.mean()), float((sens[ended] > parity.SENS_EXEMPT).mean())))
        print(what + "worst non-exempt error per block %s; of the resets: in contact %.3f, exempt %.3f; of all envs: exempt %.3f" % (
            (worst,) + shares[-1] + (float((sens > parity.SENS_EXEMPT).mean()),)))
    env.close()
    return torch.stack(rec)


def test_gpu_rearrange_auto_reset_calls_against_step_auto(parity):
    """the auto-resetting step call (k_ra_step's done list -> k_ra_reset in the same call) against step_auto from the device's
    pre-call state: who ends when, the terminal observation, the post-reset outputs and goals, the step's reward; and the same
    calls without the class order, bit for bit.  Measured on an MI355X, worst non-exempt error over the four calls: terminal obs
    1.4e-3, obs 1.3e-3, ag 7.1e-6, state 1.0e-3; of the 32 / 33 resets of a call 24 - 41 % were in contact and 13 - 22 % exempt,
    of all 129 envs of a call 4.7 - 7.8 % were exempt."""
    import torch
    ordered = _auto_reset_run(parity, "1", check=True)
    plain = _auto_reset_run(parity, "0", check=False)
    assert torch.equal(ordered, plain)


def test_gpu_rearrange_reward_kernel_matches_reference_numpy():
    import torch
    d = np.load(os.path.join(GOLDEN, "rearrange_reward_reference.npz"))
    ag, g = torch.tensor(d["achieved_goal"], dtype=torch.float32), torch.tensor(d["goal"], dtype=torch.float32)
    dist = np.linalg.norm(d["achieved_goal"] - d["goal"], axis=1)
    clear = np.abs(dist - 0.12) > 1e-5
    for rt in ("sparse", "dense"):
        env = _make(4, config={"reward_type": rt})
        out = env.compute_reward(ag, g).cpu().numpy()
        if rt == "sparse":
            assert np.array_equal(out[clear], d["reward_sparse"][clear])
        else:
            assert np.allclose(out, d["reward_dense"], atol=1e-6)
        host = R.compute_reward(d["achieved_goal"], d["goal"], 0 if rt == "sparse" else 1)   # the host build's float32 arithmetic
        assert np.array_equal(out, host) if rt == "sparse" else np.allclose(out, host, rtol=1e-6, atol=0)
        env.close()


def test_gpu_rearrange_class_order_changes_nothing_but_the_time():
    import torch
    import gym_xarm_amd
    E = 3000
    outs = []
    for flag in ("1", "0"):
        os.environ["XARM_RA_CLASS_ORDER"] = flag
        try:
            env = gym_xarm_amd.make("XarmRearrange-v0", num_envs=E, seed=4)
        finally:
            del os.environ["XARM_RA_CLASS_ORDER"]
        env.reset()
        s = env.get_state()
        s[: E // 6, R.BP:R.BP + 12] = torch.tensor([-0.05, 0.0, 0.025, 0.0, 0.0, 0.025, 0.05, 0.0, 0.025, 0.1, 0.0, 0.025], device=env.device)
        s[E // 6: E // 3, R.BP:R.BP + 12] = torch.tensor([0.0, 0.1, 0.025, 0.0, 0.1, 0.075, 0.0, 0.1, 0.125, 0.2, 0.0, 0.025], device=env.device)
        s[: E // 3, R.BQ:R.BQ + 16] = torch.tensor([0.0, 0.0, 0.0, 1.0] * 4, device=env.device)
        s[: E // 3, R.BV:R.BV + 24] = 0
        env.set_state(s)
        env.set_episode_steps(torch.arange(E, device=env.device) % 100)
        gen = torch.Generator(device=env.device)
        gen.manual_seed(2)
        rec = []
        for _ in range(8):
            a = torch.rand(E, 8, device=env.device, generator=gen) * 2 - 1
            obs, rew, done, info = env.step(a)
            rec.append(torch.cat([obs["observation"], obs["achieved_goal"], obs["desired_goal"], rew[:, None], done[:, None].float(),
                                  env.get_state()], dim=1).clone())
        if flag == "1":
            assert len(torch.unique(env.class_keys())) >= 3
        outs.append(torch.stack(rec))
        env.close()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


def test_gpu_rearrange_full_size_properties_8192():
    import torch
    E = 8192
    a = [torch.rand(E, 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(k)) * 2 - 1 for k in range(4)]

    def run(n, off):
        env = _make(n, seed=9, env_id_offset=off)
        env.reset()
        s = env.get_state()
        s[: n // 4, R.STEPS] = 48
        env.set_state(s)
        for k in range(4):
            obs, rew, done, info = env.step(a[k][off:off + n])
        out = env.get_state().clone(), obs["observation"].clone(), rew.clone(), done.clone(), env.episode_steps().clone()
        env.close()
        return out
    full, again = run(E, 0), run(E, 0)
    for x, y in zip(full, again):
        assert torch.equal(x, y)
    half = run(E // 2, E // 2)
    st, steps = full[0], full[4]
    quarter = E // 4
    assert torch.equal(st[E // 2 + E // 8:], half[0][E // 8:]) and torch.equal(full[1][E // 2 + E // 8:], half[1][E // 8:])
    assert torch.isfinite(st).all()
    q = st[:, R.BQ:R.BQ + 16].reshape(E, 4, 4)
    assert float((q.norm(dim=2) - 1).abs().max()) < 1e-5
    assert bool((st[:, R.LT:R.LP + 8] >= 0).all())
    assert bool((steps[:quarter] == 2).all()) and bool((steps[quarter:] == 4).all())
    assert bool(((full[2] == 0) | (full[2] == -1)).all())


def test_gpu_rearrange_scripted_carry_to_goal():
    """cubes 0-2 sit on their goals; arm 0 carries cube 3 to its goal: is_success 0 -> 1, reward -1 -> 0, the others stay"""
    import torch
    env = _make(1, seed=1, auto_reset=False)
    s = env.get_state()
    cubes = [[0.2, -0.1, 0.025], [0.2, 0.1, 0.025], [0.05, -0.15, 0.025], [-0.2, 0.0, 0.025]]
    goals = cubes[:3] + [[-0.2, 0.15, 0.025]]
    s[0, R.BP:R.BP + 12] = torch.tensor(sum(cubes, []), device=env.device)
    s[0, R.GOAL:R.GOAL + 12] = torch.tensor(sum(goals, []), device=env.device)
    env.set_state(s)
    obs, rew, done, info = env.step(torch.zeros(1, 8))
    assert float(rew[0]) == -1.0 and float(info["is_success"][0]) == 0.0
    o = obs["observation"].cpu().numpy()

    def servo(xy, z, g, n):
        nonlocal o, rew, info
        for _ in range(n):
            hp = o[0, 52:55]
            a = np.zeros((1, 8), np.float32)
            a[0, 0:2] = np.clip((np.asarray(xy) - hp[:2]) / 0.0625, -1, 1)
            a[0, 2] = np.clip((z - hp[2]) / 0.0625, -1, 1)
            a[0, 3] = g
            ob, rew, _, info = env.step(torch.from_numpy(a))
            o = ob["observation"].cpu().numpy()

    servo([-0.2, 0], 0.25, 1, 12); servo([-0.2, 0], 0.085, 1, 12); servo([-0.2, 0], 0.085, -1, 6); servo([-0.2, 0], 0.2, -1, 8)
    assert o[0, 11] > 0.1, "cube 3 was not lifted"
    servo([-0.2, 0.15], 0.2, -1, 12); servo([-0.2, 0.15], 0.09, -1, 10); servo([-0.2, 0.15], 0.09, 1, 6); servo([-0.2, 0.15], 0.25, 1, 8)
    c = o[0, 0:12].reshape(4, 3)
    assert np.linalg.norm(c[3] - goals[3]) < 0.05, c
    assert np.abs(c[:3] - np.asarray(cubes[:3])).max() < 2e-3
    assert float(info["is_success"][0]) == 1.0 and float(rew[0]) == 0.0
    env.close()


def test_gpu_rearrange_render_matches_stack_tower_without_cube_3():
    """cube 3 and goal 3 out of view, everything else a StackTower state: the two renders agree"""
    import torch
    import gym_xarm_amd
    st = gym_xarm_amd.make("XarmPDStackTower-v0", num_envs=4, seed=3, auto_reset=False)
    st.reset()
    st.step(torch.rand(4, 8, generator=torch.Generator().manual_seed(1)) * 2 - 1)
    s3 = st.get_state().cpu().numpy().astype(np.float64)
    ra = _make(4, seed=3, auto_reset=False)
    rows = R.from_stack(s3, 3, (0.0, 0.0))
    rows[:, R.BP + 9:R.BP + 12] = [0.0, 0.0, -5.0]        # below the floor: no camera ray reaches it
    rows[:, R.GOAL + 9:R.GOAL + 12] = [0.0, 0.0, -5.0]
    ra.set_state(torch.tensor(rows, dtype=torch.float32, device=ra.device))
    assert ra.default_camera() == st.default_camera()          # StackTower's camera
    a = st.render(width=160, height=120, env_ids=range(4), depth=True, segmentation=True)
    b = ra.render(width=160, height=120, env_ids=range(4), depth=True, segmentation=True)
    assert a["rgba"].shape[0] == 4
    assert torch.equal(a["rgba"], b["rgba"]) and torch.equal(a["depth"], b["depth"]) and torch.equal(a["seg"], b["seg"])
    # all four cubes in view: four distinct cube ids (8 + k), and a goal id for cube 3
    rows[:, R.BP + 9:R.BP + 12] = [0.1, -0.1, 0.025]
    rows[:, R.GOAL + 9:R.GOAL + 12] = [-0.1, 0.1, 0.025]
    for c in range(3):
        rows[:, R.BP + 3 * c:R.BP + 3 * c + 3] = [[-0.15, -0.1, 0.025], [0.0, 0.15, 0.025], [0.15, 0.05, 0.025]][c]
        rows[:, R.BQ + 4 * c:R.BQ + 4 * c + 4] = [0, 0, 0, 1]
    ra.set_state(torch.tensor(rows, dtype=torch.float32, device=ra.device))
    seg = ra.render(width=320, height=240, env_ids=range(4), segmentation=True)["seg"].cpu().numpy()
    for e in range(4):
        ids = set(np.unique(seg[e]).tolist())
        assert {8, 9, 10, 11} <= ids and 19 in ids, ids
    st.close(); ra.close()


def test_gpu_rearrange_her_relabelling_uses_compute_reward():
    import torch
    from gym_xarm_amd.her import HerReplayBuffer, collect
    env = _make(256, seed=3)
    buf = HerReplayBuffer(env, n_sampled_goal=4, seed=0)
    g = torch.Generator(device=env.device)
    g.manual_seed(0)
    collect(env, buf, lambda o: torch.rand(env.num_envs, env.act_dim, device=env.device, generator=g) * 2 - 1, 60)
    b = buf.sample(2048)
    rel = b["relabelled"]
    expect = env.compute_reward(b["next_achieved_goal"].contiguous(), b["desired_goal"].contiguous(), None)
    assert torch.equal(b["reward"][rel], expect[rel])
    assert b["desired_goal"].shape == (2048, 12)
    env.close()
