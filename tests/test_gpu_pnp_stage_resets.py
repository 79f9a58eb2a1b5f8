"""Resets per hand-off stage of the staged PickAndPlace step (XARM_RESET_PER_STAGE): every hand-off stage appends the
episodes that end in it to a list of its own and resets that list directly behind its hand-off, on the stage's side stream - against
the single list B, reset once after the last hand-off (XARM_RESET_PER_STAGE=0).  A re-scheduling: which list an env is in and on which
stream the list's reset runs; an env's reset does not depend on the envs it shares a wavefront with, so every bit stays.

8 256 envs: the smallest batch above step_coop_limit (8 192), i.e. the staged pipeline with the cooperative reset for the short lists and
the lane reset launched beside it.  The states, set with set_state as tests/test_gpu_pnp_stage_tables.py and test_gpu_pad_setup.py do:
  rows   0 ..  35   the grasp fixture's instants 28 .. 36 (the held object): pads loaded at step start - hand-off in stage 0;
  rows  36 ..  83   instant 22 (the open hand round the object), fingers closing at 0.9 .. 1.0 of full speed: the first pad row comes
                    alive in substeps 5 .. 9 of the first call (test_gpu_pad_setup.py measured 0.95 and 1.0 there) - stage 1;
  rows  84 .. 131   the same at 0.64 .. 0.72 of full speed (0.65 and 0.7 measured in substeps 10 .. 14) - stage 2;
  the rest          freshly reset envs under random actions: mostly the fast path (list A).
The episode step counters make a known part of each group end by time limit in the first call (49 of 50 steps done), the others one
to three calls later; the rest of the batch has its phases spread (~165 list-A resets per call)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E, CALLS = 8256, 4          # the captured step is replayed for the calls 2 - 4 (the first call of a handle runs outside the capture)
ENV_ID = "XarmPDPickAndPlace-v0"
HELD, MID, LATE = slice(0, 36), slice(36, 84), slice(84, 132)


@pytest.fixture(scope="module")
def gx():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gym_xarm_amd
    return gym_xarm_amd


def _make(gx, per_stage):
    mp = pytest.MonkeyPatch()
    mp.setenv("XARM_RESET_PER_STAGE", "1" if per_stage else "0")
    env = gx.make(ENV_ID, num_envs=E, seed=23)
    mp.undo()
    pipe = env.pipeline_info()
    assert env.stage_info() == [0, 5, 10, 15] and pipe["fast_pipeline"] and pipe["reset_overlap"] and pipe["reset_per_stage"] == per_stage
    return env


@pytest.fixture(scope="module")
def scene(gx, golden_rollout):
    """(start state [E, 54], the actions of the four calls): computed once, shared, never written"""
    g = golden_rollout
    env = _make(gx, True)
    env.reset()
    st = env.get_state().clone()
    env.close()
    gs, ga = g["grasp_states"], g["grasp_actions"]
    rows = [(t, e) for t in range(28, 37) for e in range(4)] + [(22, 1 + i % 3) for i in range(96)]
    assert len(rows) == LATE.stop
    st[:LATE.stop] = torch.as_tensor(np.stack([gs[t, e] for t, e in rows]), dtype=torch.float32, device="cuda")
    steps = (torch.arange(E, device="cuda") * 7919 % 50).float()
    steps[:LATE.stop] = torch.tensor([49.0, 48.0, 47.0, 46.0], device="cuda").repeat_interleave(3).repeat(LATE.stop // 12)   # the groups cycle env 1 - 3
    st[:, 52] = steps
    scale = torch.cat([torch.linspace(0.9, 1.0, 48), torch.linspace(0.64, 0.72, 48)]).cuda()
    gen = torch.Generator(device="cuda").manual_seed(9)
    acts = []
    for k in range(CALLS):
        a = torch.rand(E, 4, device="cuda", generator=gen) * 2 - 1
        a[:LATE.stop] = torch.as_tensor(np.stack([ga[min(t + k, ga.shape[0] - 1), e] for t, e in rows]), dtype=torch.float32, device="cuda")
        assert bool((a[MID.start:LATE.stop, 3] == -1.0).all())        # the fixture closes its fingers from instant 22 on
        a[MID.start:LATE.stop, 3] = -scale
        acts.append(a)
    return st, acts


def _record(env, out):
    obs, rew, done, info = out
    parts = [obs["observation"], obs["achieved_goal"], obs["desired_goal"], rew[:, None], done[:, None].float(), info["is_success"][:, None].float(),
             info["TimeLimit.truncated"][:, None].float(), info["terminal_observation"], env.get_state()]
    return torch.cat(parts, dim=1).clone()


def _run(gx, scene, per_stage):
    """four eager calls from the scene: (records [CALLS, E, *], list-A resets, resets per hand-off stage, hand-offs per stage)"""
    st, acts = scene
    env = _make(gx, per_stage)
    env.reset()
    env.set_state(st)
    rec, n_a, fin, handed = [], 0, np.zeros(3, np.int64), np.zeros(3, np.int64)
    for a in acts:
        rec.append(_record(env, env.step(a)))
        n_a += env.debug_counts()[0]
        ho, fb = env.debug_stage_counts()
        handed += np.array(ho)
        fin += np.array(fb)
    env.close()
    return torch.stack(rec), n_a, fin, handed


@pytest.fixture(scope="module")
def eager(gx, scene):
    return _run(gx, scene, True)


def test_per_stage_resets_equal_the_single_list_bit_for_bit(gx, scene, eager):
    rec, n_a, fin, handed = eager
    ref, ref_a, ref_fin, ref_handed = _run(gx, scene, False)
    print("per stage: list A %d, B0 / B1 / B2 %s, hand-offs per stage %s; single list: list A %d, list B %s, hand-offs %s" % (
        n_a, fin.tolist(), handed.tolist(), ref_a, ref_fin.tolist(), ref_handed.tolist()))
    assert torch.isfinite(rec).all()
    # every class of reset really happened (device counters), and the single list holds the same episodes
    assert n_a > 0 and (fin > 0).all(), (n_a, fin.tolist())
    assert ref_a == n_a and ref_fin[0] == fin.sum() and ref_fin[1:].sum() == 0 and (ref_handed == handed).all()
    done = rec[:, :, 31]
    assert int(done.sum()) == n_a + fin.sum()
    assert torch.equal(rec, ref)


def test_per_stage_resets_run_to_run(gx, scene, eager):
    again = _run(gx, scene, True)
    assert torch.equal(eager[0], again[0]) and eager[1] == again[1] and (eager[2] == again[2]).all()


def test_per_stage_resets_in_a_captured_step(gx, scene, eager):
    """one step captured on a side stream (as tests/test_gpu_parity.py::test_a_captured_step_replays_like_eager_steps) and replayed three
    times, for the calls 2 - 4: the forks to the stage streams, the resets on them and the joins behind the last reset are all inside the graph"""
    st, acts = scene
    env = _make(gx, True)
    env.reset()
    env.set_state(st)
    a = acts[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rec = [_record(env, env.step(a))]            # first call outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = env.step(a)
    for k in range(1, CALLS):
        a.copy_(acts[k])
        graph.replay()
        rec.append(_record(env, out))
    torch.cuda.synchronize()
    env.close()
    rec = torch.stack(rec)
    diff = (rec != eager[0])
    print("captured step: differing values per call %s, columns %s" % (diff.sum(dim=(1, 2)).tolist(), diff.any(dim=0).any(dim=0).nonzero().flatten().tolist()[:40]))
    assert int(eager[0][1:, :, 31].sum()) > 3 * 100          # the replayed calls reset a few hundred envs each
    assert torch.equal(rec, eager[0])
