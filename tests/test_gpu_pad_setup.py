"""The per-substep pad setup of the cooperative PickAndPlace core on the device (csrc/xarm_coop_core.h pad_columns: the row broadcast
folded into the multiply-adds, one division for the reciprocal diagonals of all pad rows, the pad columns scaled where they are made):
the 64 "grasp" and 64 "mixed" envs of tests/test_gpu_pad_sweep.py - pads loaded, arms inside their joint-limit windows, both, neither,
four envs to a wavefront - through one cooperative reset and three auto-resetting cooperative steps, against the host float32
cooperative core with that test's tolerances: 2e-3 on the envs the float64 host core shows well conditioned, the allowance of
oracle/parity.py on the rest, the same caps on exempt envs.  The setup is shared by the four cooperative kernels, so one more case
takes 8 envs through the staged hand-off kernel (k_step_coop_list_stage) with the step opened by 0, 5 and 10 fast substeps and
compares them with the same envs stepped by k_step_coop."""
import numpy as np
import pytest
import torch

E, STEPS, SEED = 64, 3, 9
ATOL = 2e-3     # tests/test_coop.py::test_gpu_coop_reset_matches_oracle_and_lane_kernel


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def device_runs(golden_rollout):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gym_xarm_amd
    env = gym_xarm_amd.make("XarmPDPickAndPlace-v0", num_envs=E, seed=SEED, auto_reset=True)
    env.reset()
    gen = torch.Generator().manual_seed(1)
    for t in range(10):
        env.step(torch.rand(E, 4, generator=gen) * 2 - 1)
    rnd = _np(env.get_state())
    g = golden_rollout
    grasp = np.concatenate([g["grasp_states"][k] for k in range(6, 38, 2)])[:E].astype(np.float32)
    assert grasp.shape[0] == E
    mixed = rnd.copy()
    mixed[1::3] = grasp[1::3][:len(mixed[1::3])]
    mixed[2::7, 1] = 2.0            # joint 2 inside its upper limit window
    mixed[5::11, 3] = -0.1          # joint 4 inside its lower limit window
    # envs with loaded pads, envs inside a limit window, and envs with both, sharing wavefronts
    loaded = np.abs(mixed[:, 42:46]).max(axis=1) > 0.1
    pushed = (mixed[:, 1] == 2.0) | (mixed[:, 3] == np.float32(-0.1))
    assert loaded.sum() >= 4 and pushed.sum() >= 8 and (loaded & pushed).any() and (~loaded & ~pushed).any()
    acts = torch.rand(STEPS, E, 4, generator=torch.Generator().manual_seed(2)) * 2 - 1
    out = {}
    for name, st0 in (("grasp", grasp), ("mixed", mixed)):
        runs = []
        for rep in range(2):
            env.set_state(torch.tensor(st0))
            env.reset()                               # all 64 through the cooperative kernel, 4 per wavefront
            states = [env.get_state().clone()]
            dones = []
            for k in range(STEPS):
                o = env.step(acts[k])
                states.append(env.get_state().clone())
                dones.append(o[2].clone())
            runs.append((states, dones))
        out[name] = (st0, runs)
    env.close()
    return out, _np(acts).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grasp", "mixed"])
def test_reset_and_steps_are_equal_from_run_to_run(device_runs, name):
    (sa, da), (sb, db) = device_runs[0][name][1]
    for k in range(STEPS + 1):
        assert torch.equal(sa[k], sb[k]), (name, k)
    for k in range(STEPS):
        assert torch.equal(da[k], db[k]), (name, k)


def _host_rollout(hostcore, st0, acts, f32):
    """one cooperative reset and the auto-resetting steps on the host core"""
    st = hostcore.coop_reset(st0, f32=f32, seed=SEED)[0]
    out = [st]
    for k in range(STEPS):
        st, _, _, _, _, done, _ = hostcore.coop_step(st, acts[k], f32=f32, seed=SEED)
        if done.any():                              # auto-reset, as the device does it
            st = hostcore.coop_reset(st, mask=done, f32=f32, seed=SEED)[0]
        out.append(st)
    return np.stack(out)


@pytest.fixture(scope="module")
def host_runs(device_runs, hostcore, parity):
    """per state set: the host float32 rollout, and the conditioning of every env measured on the reference alone - the float64 host
    core's response to a +-1e-6 perturbation of the start state (oracle/parity.py: two draws), the largest so far at every stage"""
    from concurrent.futures import ThreadPoolExecutor
    out, acts = device_runs
    jobs = {}
    for name, (st0, _) in out.items():
        s64 = st0.astype(np.float64)
        rng = np.random.default_rng(11)
        jobs[(name, "f32")] = (s64, 1)
        jobs[(name, "f64")] = (s64, 0)
        for d in range(2):
            jobs[(name, "p%d" % d)] = (parity.perturb(s64, rng), 0)
    with ThreadPoolExecutor(len(jobs)) as ex:       # the C calls release the interpreter lock
        res = dict(zip(jobs, ex.map(lambda j: _host_rollout(hostcore, j[0], acts, j[1]), jobs.values())))
    ret = {}
    for name in out:
        ref = res[(name, "f64")]
        sens = np.maximum(*[np.abs(res[(name, "p%d" % d)][:, :, parity.CONT] - ref[:, :, parity.CONT]).max(axis=2) for d in range(2)])
        ret[name] = (res[(name, "f32")], np.maximum.accumulate(sens, axis=0))        # [STEPS + 1, E]
    return ret


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["grasp", "mixed"])
def test_reset_and_steps_agree_with_the_host_float32_core(device_runs, host_runs, parity, name):
    """Device against the host float32 core at the 2e-3 of tests/test_coop.py's cooperative reset against the oracle.  That test holds
    its well-conditioned envs to the bound, and so does this one: a reset that opens the fingers on a held object is chaotic - the
    float64 host core answers a 1e-6 perturbation of such a start state with up to 33 (object spin, rad/s) and its float32 instantiation
    differs from it by up to 22 on the same envs.  Conditioning is measured on the reference alone: sens = the float64 host core's
    response to a +-1e-6 perturbation of the start state (oracle/parity.py), the largest up to the stage compared.
      WELL-CONDITIONED envs: sens <= 1e-5, i.e. the reference amplifies the 1e-6 probe at most tenfold.  They are held to the PLAIN
        2e-3.  The set must hold at least a quarter of the envs at every stage, among them envs that start with a
        finger on the object (pad rows) and, in the mixed states, envs that start inside a joint-limit window (arm-limit rows).
      the rest: 2e-3 + min(300 sens, 1e-2), exempt (and counted: at most half) where sens > 1e-2 / 3 - the rule of oracle/parity.py."""
    out, _ = device_runs
    st0, runs = out[name]
    dev = np.stack([_np(s).astype(np.float64) for s in runs[0][0]])
    host, sens = host_runs[name]
    assert np.isfinite(dev).all()
    # the reset carried pad rows: envs start with loaded pads
    assert (np.abs(st0[:, 42:46]).max(axis=1) > 0.1).sum() >= 4
    touching = st0[:, 50] != 0
    pushed = (st0[:, 1] == 2.0) | (st0[:, 3] == np.float32(-0.1))
    err = np.abs(dev[:, :, parity.CONT] - host[:, :, parity.CONT]).max(axis=2)          # [STEPS + 1, E]
    well = sens <= 10 * parity.EPS
    exempt = sens > parity.SENS_EXEMPT
    bound = np.where(well, ATOL, ATOL + np.minimum(parity.K_SENS * sens, parity.ALLOW_CAP))
    for k in range(STEPS + 1):
        w, r = well[k], ~well[k] & ~exempt[k]
        print("%s, %s: device vs host float32 core, max |diff| of state[:31]: %.3e over the %d well-conditioned envs (%d touching, %d in a "
              "limit window; plain %.0e), %.3e over the %d others held to a bound, %.3e over all; %d exempt (max sens %.2e)" % (
                  name, "reset" if k == 0 else "step %d" % k, err[k][w].max() if w.any() else 0.0, w.sum(), (w & touching).sum(),
                  (w & pushed).sum(), ATOL, err[k][r].max() if r.any() else 0.0, r.sum(), err[k].max(), exempt[k].sum(), sens[k].max()))
    for k in range(STEPS + 1):
        # episode bookkeeping and the counter RNG's draws (goal): exact, in every env
        assert np.array_equal(dev[k][:, 52:54], host[k][:, 52:54]), (name, k)
        np.testing.assert_allclose(dev[k][:, 31:34], host[k][:, 31:34], atol=1e-6)
        assert well[k].sum() >= E // 4 and (well[k] & touching).sum() >= 2, (name, k, well[k].sum(), (well[k] & touching).sum())
        if name == "mixed":
            assert (well[k] & pushed).sum() >= 2, (name, k)
        assert exempt[k].mean() <= 0.5, (name, k, exempt[k].mean())
        bad = np.where(~exempt[k] & (err[k] > bound[k]))[0]
        assert bad.size == 0, (name, k, bad.tolist(), err[k][bad].tolist(), sens[k][bad].tolist(), well[k][bad].tolist())


# ---- the staged hand-off kernel: 8 envs, hand-offs that continue a step from substep 0, 5 and 10
E8, STEPS8 = 8, 3
ENV_ID = "XarmPDPickAndPlace-v0"


def _handle(gx, ticks=None, stages=None, **kw):
    mp = pytest.MonkeyPatch()
    if ticks:
        mp.setenv("XARM_HO_STAGE_TICKS", ticks)
    if stages:
        mp.setenv("XARM_PNP_STAGES", str(stages))
    env = gx.make(ENV_ID, num_envs=E8, seed=41, auto_reset=False, **kw)
    mp.undo()
    return env


@pytest.mark.gpu
def test_staged_hand_off_from_substep_0_5_and_10_against_k_step_coop(golden_rollout):
    """8 envs from instant 22 of the grasp fixture (envs 1 - 3: the open hand round the object, no pad row alive yet), each closing its
    fingers at another speed (gripper action -1 ... -0.45), so that the substep in which the first pad row comes alive differs from env
    to env: at full speed it lies in [5, 10), at 0.45 - 0.7 of it in [10, 15) or in the next step; from the step after, the pads are
    loaded at step start (hand-off in stage 0).  Stage table 0|5|10|15 (XARM_HO_STAGE_TICKS, batch above step_coop_limit = 1, as
    tests/test_gpu_pnp_stage_tables.py sets it): an env is handed to k_step_coop_list_stage with tick0 = the first substep of the
    stage in which a pad row came alive.  Reference: the same states stepped by k_step_coop (batch within step_coop_limit).
      tick0 = 0: the whole step on the cooperative core in both - the same bits;
      tick0 = 5, 10: the step was opened by 5 or 10 substeps of the one-env-per-lane fast core, which sums in another order -
        float32 rounding of pad-free substeps, held to the 1e-3 on the continuous state that tests/test_gpu_pnp_stage_tables.py and
        test_gpu_parity.py::test_staged_pipeline_against_the_unstaged_one use for late hand-offs, here for every env;
      no hand-off: the fast core all step, same 1e-3.
    Which stage handed an env off is read from two-stage tables as in tests/test_gpu_pnp_stage_tables.py: against the unstaged
    pipeline an env differs under 0|10|15 when its pads came alive in [10, 15), under 0|5|15 when in [5, 15)."""
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gym_xarm_amd as gx
    fast = dict(step_coop_limit=1, reset_coop_limit=-1)
    coop = _handle(gx, step_coop_limit=E8, reset_coop_limit=E8)                      # k_step_coop
    plain = _handle(gx, stages=1, **fast)                                             # unstaged pipeline
    two5, two10 = _handle(gx, ticks="5", stages=2, **fast), _handle(gx, ticks="10", stages=2, **fast)
    staged = _handle(gx, ticks="5,10", **fast)
    assert staged.stage_info() == [0, 5, 10, 15] and two5.stage_info() == [0, 5, 15] and two10.stage_info() == [0, 10, 15] and plain.stage_info() == [0, 15]
    g = golden_rollout
    rows = [(22, 1), (22, 2), (22, 3), (22, 1), (22, 2), (22, 3), (22, 1), (22, 2)]
    scale = torch.tensor([1.0, 0.95, 0.7, 0.65, 0.6, 0.55, 0.5, 0.45], device="cuda")
    staged.reset()
    st = staged.get_state().clone()
    st[:] = torch.as_tensor(np.stack([g["grasp_states"][t, e] for t, e in rows]), dtype=torch.float32, device="cuda")
    st[:, 52] = 0
    staged.set_state(st)
    n0 = n5 = n10 = nfast = 0
    for k in range(STEPS8):
        a = torch.as_tensor(np.stack([g["grasp_actions"][t + k, e] for t, e in rows]), dtype=torch.float32, device="cuda")
        assert bool((a[:, 3] == -1.0).all())                          # the fixture closes its fingers from instant 22 on
        a[:, 3] = -scale
        st0 = staged.get_state().clone()
        out = {}
        for name, env in (("coop", coop), ("plain", plain), ("two5", two5), ("two10", two10), ("staged", staged)):
            env.set_state(st0)
            o = env.step(a)
            out[name] = (env.get_state().clone(), o[0]["observation"].clone(), o[1].clone(), o[2].clone())
        ref, stg = out["coop"], out["staged"]
        handed = (out["plain"][0] == ref[0]).all(dim=1)              # the unstaged pipeline ran the step on the cooperative core
        ge5 = ~(out["two5"][0] == out["plain"][0]).all(dim=1)        # pads came alive in [5, 15)
        ge10 = ~(out["two10"][0] == out["plain"][0]).all(dim=1)      # ... in [10, 15)
        t0 = handed & ~ge5
        t5 = ge5 & ~ge10
        t10 = ge10
        d = (stg[0] - ref[0])[:, :31].abs().max(dim=1).values
        print("step %d: hand-off from substep 0: %s, 5: %s, 10: %s, none: %s; max |d| vs k_step_coop %s" % (
            k, t0.nonzero().flatten().tolist(), t5.nonzero().flatten().tolist(), t10.nonzero().flatten().tolist(),
            (~handed & ~ge5).nonzero().flatten().tolist(), ["%.2e" % x for x in d.tolist()]))
        assert torch.isfinite(stg[0]).all()
        assert bool((ge5 | ~ge10).all())                              # [10, 15) lies in [5, 15)
        # tick0 = 0: the same bits, outputs included
        for i in range(4):
            assert torch.equal(stg[i][t0], ref[i][t0]), (k, i)
        assert float(d.max()) < 1e-3, (k, d.tolist())
        assert torch.equal(stg[3], ref[3])
        n0 += int(t0.sum()); n5 += int(t5.sum()); n10 += int(t10.sum()); nfast += int((~handed & ~ge5).sum())
        staged.set_state(stg[0])
    print("hand-offs from substep 0: %d, 5: %d, 10: %d; steps on the fast path: %d" % (n0, n5, n10, nfast))
    assert n0 > 0 and n5 > 0 and n10 > 0
    for e in (coop, plain, two5, two10, staged):
        e.close()
