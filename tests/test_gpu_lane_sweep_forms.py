"""The two forms of the lane sweep (csrc/xarm_core.h xk::substep; tests/test_lane_sweep_forms.py holds them to each other on the host) on
the device: the product library against a variant of the same tree built with -DXK_SWEEP_V1 -DXK_TABLE_V1 - one set of impulses and a copy
per row, one loop with a test per arm-limit row.  Same arithmetic in the same order, and the forms differ in nothing the compiler may
contract differently, so every bit stays.

512 PickAndPlace envs with step_coop_limit = 1 (the 'fast' family of gym_xarm_amd.distributed.reproducible_limits): the fast stages, the
hand-offs and the lane kernels run at this size as they do at 65 536.  Desynchronised phases (time-limit resets in every call), auto-reset
on, 12 calls of seeded random actions.  The variant runs in a fresh child process that names it in XARM_HIP_LIB (a process binds one
library); it is built once, beside the product library, and reused while no source is newer."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, CALLS, SEED = 512, 12, 31
ENV_ID = "XarmPDPickAndPlace-v0"
V1_FLAGS = ["-DXK_SWEEP_V1", "-DXK_TABLE_V1"]


def _rollout():
    """12 calls on the library this process binds: dict of arrays [CALLS, E, *] and the device counters"""
    import torch
    import gym_xarm_amd as gx
    from gym_xarm_amd import _native, distributed as D
    limits = D.reproducible_limits(E, "fast")
    assert limits["step_coop_limit"] == 1
    env = gx.make(ENV_ID, num_envs=E, seed=SEED, **limits)
    assert env.stage_info() == [0, 5, 10, 15] and env.pipeline_info()["fast_pipeline"]
    env.reset()
    env.set_episode_steps(torch.arange(E, device="cuda") * 7919 % 50)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    ring = [torch.rand(E, 4, device="cuda", generator=gen) * 2 - 1 for _ in range(CALLS)]
    obs_l, rew_l, done_l, st_l = [], [], [], []
    ended, handed, fin = 0, np.zeros(3, np.int64), np.zeros(3, np.int64)
    for a in ring:
        obs, rew, done, _ = env.step(a)
        obs_l.append(torch.cat([obs["observation"], obs["achieved_goal"], obs["desired_goal"]], dim=1).cpu().numpy())
        rew_l.append(rew.cpu().numpy())
        done_l.append(done.cpu().numpy())
        st_l.append(env.get_state().cpu().numpy())
        ended += env.debug_counts()[0]
        ho, fb = env.debug_stage_counts()
        handed += np.array(ho)
        fin += np.array(fb)
    env.close()
    return dict(obs=np.stack(obs_l), reward=np.stack(rew_l), done=np.stack(done_l), state=np.stack(st_l), ended=np.int64(ended), handed=handed,
                fin=fin, lib=np.array(os.path.realpath(_native.loaded_path())))


if __name__ == "__main__":      # the child process: python tests/test_gpu_lane_sweep_forms.py OUT.npz, with XARM_HIP_LIB set
    sys.path.insert(0, ROOT)
    np.savez(sys.argv[1], **_rollout())
    sys.exit(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def v1_lib():
    """csrc/libxarm_hip_sweep_v1.so: the tree's library with the lane sweep in its first form"""
    from gym_xarm_amd import build as B
    lib = os.path.join(B.CSRC, "libxarm_hip_sweep_v1.so")
    deps = [os.path.join(B.CSRC, s) for s in B.SOURCES] + [os.path.join(ROOT, "include", "xarm_hip.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps if os.path.exists(d)):
        if not (os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
            pytest.skip("hipcc is needed to build the first-form variant of the library")
        B.build(force=True, verbose=False, lib=lib, extra_flags=V1_FLAGS)
    return lib


def test_product_sweep_equals_the_first_form_on_the_device(v1_lib, tmp_path):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from gym_xarm_amd import _native
    assert not os.environ.get("XARM_HIP_LIB"), "this process must bind the product library"
    out = str(tmp_path / "v1.npz")
    child = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, XARM_HIP_LIB=v1_lib, PYTHONPATH=ROOT),
                           cwd=ROOT, capture_output=True, text=True)
    assert child.returncode == 0, child.stderr[-3000:]
    ref = np.load(out)
    got = _rollout()
    assert str(ref["lib"]) == os.path.realpath(v1_lib) and str(got["lib"]) == os.path.realpath(_native.LIB_PATH)
    print("hand-offs per stage %s, episodes ended in the fast stages %d, in the hand-offs per stage %s" % (
        got["handed"].tolist(), int(got["ended"]), got["fin"].tolist()))
    # the fast stages, every stage's hand-off and the resets behind both were at work
    assert (got["handed"] > 0).all() and got["ended"] > 0 and got["fin"].sum() > 0
    assert int(got["done"].sum()) == got["ended"] + got["fin"].sum()
    for k in ("handed", "fin", "ended"):
        assert np.array_equal(got[k], ref[k]), k
    for k in ("obs", "reward", "done", "state"):
        assert np.isfinite(got[k].astype(np.float64)).all(), k
        assert got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), k
