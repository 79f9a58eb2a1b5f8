"""The kernel's restructured algorithm (csrc/xarm_core.h: world-frame CRBA + Cholesky, operational-
space block PGS, lane-masked execution) compiled for the host and compared with the oracle.  In
float64 the two must agree to rounding - they are the same Gauss-Seidel sweep in exact arithmetic -
which is what licenses the float32 tolerance used on the GPU."""
import ctypes as C

import numpy as np
import pytest


def test_ik_matches_oracle(oracle, hostcore):
    rng = np.random.default_rng(3)
    for _ in range(20):
        q = np.concatenate([rng.uniform(-0.5, 0.5, 7) + [0, 0.2, 0, 0.8, 0, 0.6, 0], [0.02, 0.02]])
        tgt = rng.uniform([0.3, -0.3, 0.15], [0.5, 0.3, 0.4])
        ref = oracle.ik(q, tgt, 15)
        np.testing.assert_allclose(hostcore.ik(q, tgt, f32=0), ref, atol=1e-10)
        np.testing.assert_allclose(hostcore.ik(q, tgt, f32=1), ref, atol=5e-4)


def test_init_and_reset_match_oracle(oracle, hostcore):
    E = 16
    ora = oracle.OraclePnP(E, seed=21, goal_ground_rate=0.5, init_grasp_rate=0.25)
    kw = dict(seed=21, ggr=0.5, igr=0.25)
    st0 = hostcore.init(E, f32=0, **kw)
    np.testing.assert_allclose(st0, ora.state, atol=1e-15)
    st32 = hostcore.init(E, f32=1, **kw)
    np.testing.assert_allclose(st32, ora.state, atol=1e-7)
    o_obs, o_ag, o_dg = ora.reset()
    st, obs, ag, dg = hostcore.reset(st0, f32=0, **kw)
    np.testing.assert_allclose(st, ora.state, atol=1e-9)
    np.testing.assert_allclose(obs, o_obs, atol=1e-9)
    # masked reset leaves the other envs untouched
    mask = np.zeros(E, np.uint8)
    mask[::3] = 1
    st2, *_ = hostcore.reset(st, mask=mask, f32=0, **kw)
    assert np.array_equal(st2[mask == 0], st[mask == 0])
    assert (st2[mask == 1, 53] == 2).all() and (st2[mask == 1, 52] == 0).all()


@pytest.mark.parametrize("key", ["rand", "grasp"])
def test_step_f64_equals_oracle_on_golden_rollout(hostcore, golden_rollout, parity, key):
    g = golden_rollout
    S, A = g[key + "_states"], g[key + "_actions"]
    seed = 7 if key == "rand" else 1
    worst, n_ok = 0.0, 0
    for t in range(A.shape[0]):
        st, obs, ag, dg, rew, done, succ = hostcore.step(S[t], A[t], f32=0, seed=seed)
        sens = g[key + "_sens"][t]
        err = np.abs(st - S[t + 1]).max(axis=1)
        # identical algorithm in exact arithmetic: rounding-level agreement, scaled by conditioning
        ok = sens < 1e-2   # sens >= SENS_EXEMPT marks transitions on a contact-geometry discontinuity
        assert (err[ok] <= 1e-9 + 1e-4 * sens[ok]).all(), (t, err[ok].max())
        n_ok += ok.sum()
        np.testing.assert_allclose(obs[ok], g[key + "_obs"][t][ok], atol=1e-8)
        assert np.array_equal(rew[ok], g[key + "_rew"][t][ok])
        assert np.array_equal(done[ok], g[key + "_done"][t][ok])
        worst = max(worst, err[ok].max())
    assert worst < 1e-9
    assert n_ok >= 0.85 * A.shape[0] * A.shape[1]


@pytest.mark.parametrize("key", ["rand", "grasp"])
def test_step_f32_within_conditioned_tolerance(hostcore, golden_rollout, parity, key):
    g = golden_rollout
    S, A = g[key + "_states"], g[key + "_actions"]
    seed = 7 if key == "rand" else 1
    for t in range(A.shape[0]):
        st, obs, *_ = hostcore.step(S[t], A[t], f32=1, seed=seed)
        parity.compare(st[:, parity.CONT], S[t + 1][:, parity.CONT], g[key + "_sens"][t], what="%s t=%d" % (key, t),
                       frac_tight=0.9 if key == "rand" else 0.75, max_exempt=0.15 if key == "rand" else 0.25)


def test_substeps_with_contact_f32(hostcore, golden_rollout):
    """well-conditioned grasp states (object held between the pads): 15 substeps toward fixed targets"""
    g = golden_rollout
    S = g["grasp_states"][-3]
    held = S[:, 20] > 0.15
    assert held.any()
    qt = S[:, :9].copy()
    a = hostcore.substep(S[held], qt[held], 15, f32=0)
    b = hostcore.substep(S[held], qt[held], 15, f32=1)
    assert np.abs(a[:, 42:50]).max() > 1e-3          # pads really carry load
    np.testing.assert_allclose(b[:, :31], a[:, :31], atol=2e-4)


def test_time_limit_and_auto_counter(hostcore):
    st = hostcore.init(4, f32=1, seed=2)
    st, *_ = hostcore.reset(st, f32=1, seed=2)
    for k in range(50):
        st, obs, ag, dg, rew, done, succ = hostcore.step(st, np.zeros((4, 4)), f32=1, seed=2)
        assert (st[:, 52] == k + 1).all()
        assert (done == ((k == 49) | (succ == 1))).all()


def test_dense_reward_f64_matches_oracle(oracle, hostcore, golden_rollout):
    g = golden_rollout
    S, A = g["grasp_states"], g["grasp_actions"]
    ora = oracle.OraclePnP(S.shape[1], seed=1, reward_type="dense")
    for t in range(0, A.shape[0], 3):
        ora.set_state(S[t])
        o = ora.step(A[t])
        st, obs, ag, dg, rew, done, succ = hostcore.step(S[t], A[t], f32=0, seed=1, rt=2)
        ok = g["grasp_sens"][t] < 1e-2
        np.testing.assert_allclose(rew[ok], o[3][ok], atol=1e-9)


def test_fast_step_is_the_plain_step_for_every_env_it_accepts(hostcore, golden_rollout):
    """xk::env_step_fast (the pad-free substep behind k_step_fast_stage, as its one stage [0, 15)): on every env it accepts the result is the plain
    env_step's bit for bit - state, observation, reward, done - in float32 and in float64; an env it rejects (a finger-pad
    row became active) comes back untouched; and no env that ends the step with a pad impulse is ever accepted"""
    g = golden_rollout
    for key in ("rand", "grasp"):
        S, A = g[key + "_states"], g[key + "_actions"]
        n_ok = n_all = 0
        for t in range(0, A.shape[0], 2):
            for f32 in (0, 1):
                a = hostcore.step(S[t], A[t], f32=f32)
                b = hostcore.step_fast(S[t], A[t], f32=f32)
                ok = b[7]
                assert np.array_equal(b[0][ok], a[0][ok]) and np.array_equal(b[1][ok], a[1][ok])
                assert np.array_equal(b[4][ok], a[4][ok]) and np.array_equal(b[5][ok], a[5][ok]) and np.array_equal(b[6][ok], a[6][ok])
                assert np.array_equal(b[0][~ok], S[t][~ok])
                pad = (a[0][:, 42:46] != 0).any(axis=1)
                assert not (pad & ok).any()
            n_ok += ok.sum()
            n_all += ok.size
        assert (0.85 < n_ok / n_all <= 1.0) if key == "rand" else (0.4 < n_ok / n_all < 0.9)   # the grasp script lives in contact


def _pnp_staged(hostcore, state, actions, stages, f32):
    """xh_pnp_staged (tests/hostbuild/xarm_host.cpp): the staged pipeline of xarm_step; stage 0 = finished on the fast path,
    1 + c = handed off to the cooperative rows in stage c"""
    E = state.shape[0]
    st = np.array(state, dtype=np.float64, copy=True)
    a = np.ascontiguousarray(actions, dtype=np.float64)
    obs, rew = np.zeros((E, 24)), np.zeros(E)
    done, succ, stage = np.zeros(E, np.uint8), np.zeros(E, np.uint8), np.zeros(E, np.uint8)
    hostcore.L.xh_pnp_staged(C.c_int(f32), *hostcore._cfg(), C.c_int64(E), C.c_int(stages), hostcore._p(st), hostcore._p(a), hostcore._p(obs),
                             hostcore._p(rew), hostcore._u8(done), hostcore._u8(succ), hostcore._u8(stage))
    return st, obs, rew, done, succ, stage


def test_staged_pipeline_f64_equals_oracle_and_hands_off_late_contacts_late(hostcore, golden_rollout):
    """PickAndPlace's staged step (fast stages of xk::env_step_fast_range on a copy; the stage that sees a pad row is dropped and
    xc::env_step_from finishes the step from its first substep) - the host counterpart of the Handover test of the same name.
    Three stages in float64 == the oracle's next state within the bound of test_step_f64_equals_oracle_on_golden_rollout; one stage
    is step_fast on the envs that accepts and coop_step on the others, bit for bit; three stages are one stage bit for bit on every
    env that finishes fast or is handed off in stage 0; over the random rollout the fast path and a hand-off in each of the three
    stages all occur (a contact that begins late in the step is handed off late)."""
    g = golden_rollout
    for key in ("rand", "grasp"):
        S, A = g[key + "_states"], g[key + "_actions"]
        seen = np.zeros(4, np.int64)
        worst, n_ok = 0.0, 0
        for t in range(A.shape[0]):
            st, obs, rew, done, succ, stage = _pnp_staged(hostcore, S[t], A[t], 3, f32=0)
            sens = g[key + "_sens"][t]
            err = np.abs(st - S[t + 1]).max(axis=1)
            ok = sens < 1e-2
            print(key, t, "worst non-exempt err", err[ok].max(), "stages", np.bincount(stage, minlength=4))
            assert (err[ok] <= 1e-9 + 1e-4 * sens[ok]).all(), (t, err[ok].max())
            n_ok += ok.sum()
            np.testing.assert_allclose(obs[ok], g[key + "_obs"][t][ok], atol=1e-8)
            assert np.array_equal(rew[ok], g[key + "_rew"][t][ok])
            assert np.array_equal(done[ok], g[key + "_done"][t][ok])
            worst = max(worst, err[ok].max())
            seen += np.bincount(stage, minlength=4)
            for f32 in (0, 1):
                three = st, obs, rew, done, succ, stage
                if f32:
                    three = _pnp_staged(hostcore, S[t], A[t], 3, f32=1)
                one = _pnp_staged(hostcore, S[t], A[t], 1, f32=f32)
                fast = hostcore.step_fast(S[t], A[t], f32=f32)
                acc = fast[7]
                coop = hostcore.coop_step(S[t][~acc], A[t][~acc], f32=f32)     # only the envs the fast step refused
                assert np.array_equal(one[5] == 0, acc)
                same = three[5] <= 1
                assert np.array_equal(three[5][same], one[5][same])
                for k, j in enumerate((0, 1, 4, 5, 6)):      # state, obs, reward, done, success
                    assert np.array_equal(one[k][acc], fast[j][acc]) and np.array_equal(one[k][~acc], coop[j]), (key, t, f32, k)
                    assert np.array_equal(three[k][same], one[k][same]), (key, t, f32, k)
        print(key, "stage census", seen, "worst", worst, "non-exempt share", n_ok / (A.shape[0] * A.shape[1]))
        assert worst < 1e-9
        assert n_ok >= 0.85 * A.shape[0] * A.shape[1]
        if key == "rand":
            assert (seen > 0).all(), seen        # fast path, and a hand-off in each of the three stages
