"""Front-loaded stage tables of the pipelined PickAndPlace step (10|13 and 11|13, set through XARM_HO_STAGE_TICKS) against the unstaged
pipeline (XARM_PNP_STAGES=1) from identical states, on 256 envs = 4 fast wavefronts, with the handles built the way the `fast` family
of tests/test_gpu_parity.py builds them.

The batch mixes the scripted grasp fixture (every instant of its four envs: approach, closing fingers, the held object) with freshly
reset envs under random actions, so that pads come alive at step start (hand-off in stage 0), in the middle of a step (later stages)
and not at all (the fast path).  The C ABI reports the number of hand-offs of a call, not which env left in which stage, so the envs
are told apart by their states:
  held   pad impulses above 0.1 at the start of the step: the pad rows are active in substep 0 - handed off in stage 0;
  far    the object further than 0.25 m from the hand after the step (a step moves the hand by centimetres): no pad row all step -
         the fast path.
Both sets run the same code over the same substeps staged and unstaged and must match BIT FOR BIT.  Every other env may have been
handed off late (its first substeps on the lane core instead of the cooperative one) and is held to the tolerance of
test_gpu_parity.py::test_staged_pipeline_against_the_unstaged_one: |d| < 1e-3 over the continuous state for more than 99.5 % of the
batch.  That late hand-offs happen in BOTH later stages is shown with two-stage tables: the envs that differ from the unstaged step
under the table 0|13|15 are handed off in [13, 15), those that differ under 0|10|15 in [10, 15)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, STEPS = 256, 10
ENV_ID = "XarmPDPickAndPlace-v0"


@pytest.fixture(scope="module")
def gx():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gym_xarm_amd
    return gym_xarm_amd


def _make(gx, **kw):
    """the `fast` family of tests/test_gpu_parity.py: every batch of more than one env on the fast pipeline, resets on k_reset"""
    kw.setdefault("step_coop_limit", 1)
    kw.setdefault("reset_coop_limit", -1)
    return gx.make(ENV_ID, num_envs=E, **kw)


def _fixture_states(env, golden_rollout):
    """rows 0 .. 147: the grasp fixture's 37 instants x 4 envs; the rest: what reset() gave.  Returns the states and, per row, the
    fixture instant it starts from (-1: a reset env)"""
    g = golden_rollout
    S = torch.as_tensor(g["grasp_states"].reshape(-1, 54), dtype=torch.float32, device="cuda")
    st = env.get_state().clone()
    st[:S.shape[0]] = S
    st[:, 52] = 0                                        # episode step counters: no time limit inside the test
    t0 = np.full(E, -1)
    t0[:S.shape[0]] = np.repeat(np.arange(37), 4)
    return st, t0


def _actions(golden_rollout, t0, k, gen):
    """the fixture's own script for its rows (instant t0 + k, held at the last one), uniform random for the reset envs"""
    a = torch.rand(E, 4, device="cuda", generator=gen) * 2 - 1
    ga = golden_rollout["grasp_actions"]
    rows = np.nonzero(t0 >= 0)[0]
    t = np.minimum(t0[rows] + k, ga.shape[0] - 1)
    a[torch.as_tensor(rows, device="cuda")] = torch.as_tensor(ga[t, rows % 4], dtype=torch.float32, device="cuda")
    return a


@pytest.fixture(scope="module")
def unstaged(gx, golden_rollout):
    """the unstaged pipeline's handle, shared by the tables under test (it is only ever stepped from states set into it)"""
    mp = pytest.MonkeyPatch()
    mp.setenv("XARM_PNP_STAGES", "1")
    env = _make(gx, seed=41, auto_reset=False)
    mp.undo()
    assert env.stage_info() == [0, 15]
    yield env
    env.close()


def _staged(gx, ticks, stages=None, **kw):
    mp = pytest.MonkeyPatch()
    mp.setenv("XARM_HO_STAGE_TICKS", ticks)
    if stages:
        mp.setenv("XARM_PNP_STAGES", str(stages))
    env = _make(gx, **kw)
    mp.undo()
    return env


@pytest.mark.parametrize("ticks", ["10,13", "11,13"])
def test_front_loaded_table_against_the_unstaged_pipeline(gx, unstaged, golden_rollout, ticks):
    t1, t2 = (int(x) for x in ticks.split(","))
    staged = _staged(gx, ticks, seed=41, auto_reset=False)
    two_a, two_b = _staged(gx, str(t1), stages=2, seed=41, auto_reset=False), _staged(gx, str(t2), stages=2, seed=41, auto_reset=False)
    assert staged.stage_info() == [0, t1, t2, 15] and two_a.stage_info() == [0, t1, 15] and two_b.stage_info() == [0, t2, 15]
    staged.reset()
    st, t0 = _fixture_states(staged, golden_rollout)
    staged.set_state(st)
    gen = torch.Generator(device="cuda").manual_seed(77)
    n_held = n_far = n_late = n_handed = n_from_t1 = n_from_t2 = 0
    worst_frac, worst_d = 1.0, 0.0
    for k in range(STEPS):
        a = _actions(golden_rollout, t0, k, gen)
        st0 = staged.get_state().clone()
        unstaged.set_state(st0)
        obs, rew, done, _ = staged.step(a)
        ref, handed = staged.get_state().clone(), staged.debug_counts()[1]
        pobs, prew, pdone, _ = unstaged.step(a)
        plain = unstaged.get_state().clone()
        assert abs(unstaged.debug_counts()[1] - handed) <= 0.02 * handed + 2         # the same envs are handed off (but for borderline pads)
        same = (ref == plain).all(dim=1)
        held = st0[:, 42:50].abs().max(dim=1).values > 0.1
        far = pobs["observation"][:, 21:24].norm(dim=1) > 0.25
        # stage-0 hand-offs and fast-path envs: the same bits, outputs included
        must = held | far
        assert bool(same[must].all()), (k, int((~same & held).sum()), int((~same & far).sum()))
        assert torch.equal(rew[same], prew[same]) and torch.equal(done[same], pdone[same]) and torch.equal(obs["observation"][same], pobs["observation"][same])
        # late hand-offs: the tolerance of test_staged_pipeline_against_the_unstaged_one
        d = (ref - plain)[:, :31].abs().max(dim=1).values
        frac = float((d < 1e-3).float().mean())
        worst_frac, worst_d = min(worst_frac, frac), max(worst_d, float(d.max()))
        print("table %s step %d: handed %d, differ %d, max |d| %.3g, frac(|d| < 1e-3) %.4f" % (ticks, k, handed, int((~same).sum()), float(d.max()), frac))
        assert frac > 0.995, (k, float(d.max()), frac)
        assert handed >= int(held.sum())
        n_held += int(held.sum()); n_far += int(far.sum()); n_late += int((~same).sum()); n_handed += handed
        # which later stage the late hand-offs fall into: two-stage tables from the same state
        for env2, name in ((two_a, "a"), (two_b, "b")):
            env2.set_state(st0)
            env2.step(a)
            diff = int((~(env2.get_state() == plain).all(dim=1)).sum())
            if name == "a":
                n_from_t1 += diff
            else:
                n_from_t2 += diff
        staged.set_state(st0)                                                       # run to run
        staged.step(a)
        assert torch.equal(staged.get_state(), ref)
    print("table %s: held %d, far %d, handed %d, late %d (from tick %d: %d, from tick %d: %d), worst frac %.4f, worst |d| %.3g" % (
        ticks, n_held, n_far, n_handed, n_late, t1, n_from_t1, t2, n_from_t2, worst_frac, worst_d))
    # hand-offs in every stage: stage 0 (held), stage 2 (differ under 0|t2|15), stage 1 (more differ under 0|t1|15 than under 0|t2|15)
    assert n_held > 0 and n_far > 0 and n_handed > n_held
    assert n_from_t2 > 0 and n_from_t1 > n_from_t2 and n_late > 0
    for e in (staged, two_a, two_b):
        e.close()


@pytest.mark.parametrize("ticks", ["10,13", "11,13"])
def test_front_loaded_table_is_reproducible_with_auto_reset(gx, golden_rollout, ticks):
    """two runs with auto-reset on, from one state with the episode phases spread (five resets per call): the same bits"""
    env = _staged(gx, ticks, seed=42)
    assert env.stage_info() == [0] + [int(x) for x in ticks.split(",")] + [15]
    env.reset()
    s0, t0 = _fixture_states(env, golden_rollout)
    s0[:, 52] = (torch.arange(E, device="cuda") * 7919 % 50).float()
    outs, n_done = [], 0
    for rep in range(2):
        env.set_state(s0)
        gen = torch.Generator(device="cuda").manual_seed(5)
        rec = []
        for k in range(6):
            obs, rew, done, info = env.step(_actions(golden_rollout, t0, k, gen))
            rec.append(torch.cat([obs["observation"], rew[:, None], done[:, None].float(), env.get_state()], dim=1).clone())
            n_done += int(done.sum())
        outs.append(torch.stack(rec))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    assert n_done >= 2 * 6 * 4                            # resets really happened in every call
    env.close()
