"""The pad and arm-limit rows of the cooperative PickAndPlace sweep on the device (csrc/xarm_coop_core.h sweep_all: friction limit from
the fresh normal impulse, commit-free pad rows, the loop without per-pad tests): 64 envs from the "grasp" and "mixed" states of
tests/test_coop.py::test_gpu_coop_reset_is_deterministic_and_neighbour_independent - pads loaded, arms inside their joint-limit
windows, both, neither, four envs to a wavefront, so one launch mixes the pad-only, the arm-limit-only and the pad + arm-limit
instantiations - through one cooperative reset and three auto-resetting steps: equal from run to run, and equal to the host float32
cooperative core within the tolerance tests/test_coop.py uses for the device's cooperative reset against the oracle (2e-3 on
joints, joint velocities and object pose / twist) on the well-conditioned envs, with the conditioning allowance of oracle/parity.py
where the reference itself is ill-conditioned (a reset that opens the fingers on a held object)."""
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
