"""The two forms of the cooperative pair sweep (csrc/xarm_coop_core.h sweep_all): one set of the 14 impulse pairs with a copy per
pair step (-DXC_SWEEP_COPY, the earlier form) against two sets that the sweeps read and write in turn (the product).  Same
arithmetic in the same order, so the two host builds must agree BIT FOR BIT, in float32 and float64, with an even sweep count
(the product's) and with an odd one (the epilogue sweep; the final gather then reads the other set)."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostbuild", "xarm_sweep_host.cpp")
E, STEPS = 32, 20


JOBS = {"two": [], "copy": ["-DXC_SWEEP_COPY"], "two_odd": ["-DXC_SWEEP_ITERS=49"], "copy_odd": ["-DXC_SWEEP_COPY", "-DXC_SWEEP_ITERS=49"]}


def _build(name):
    """tests/hostbuild/libxarm_sweep_<name>.so, rebuilt when a source is newer (as conftest.HostCore keeps libxarm_host.so)"""
    so = os.path.join(os.path.dirname(SRC), "libxarm_sweep_%s.so" % name)
    srcs = [SRC] + [os.path.join(ROOT, "gym_xarm_amd", "csrc", f) for f in ("xarm_core.h", "xarm7_pd_model.h", "xarm_coop_core.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs):
        # -Og: a third of the compile time of -O1; the comparison is between builds of the same flags
        subprocess.check_call(["g++", "-Og", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas"] + JOBS[name] + ["-o", so, SRC])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def builds():
    with ThreadPoolExecutor(len(JOBS)) as ex:
        libs = dict(zip(JOBS, ex.map(_build, JOBS)))
    assert (libs["two"].xsw_sets(), libs["copy"].xsw_sets(), libs["two_odd"].xsw_sets(), libs["copy_odd"].xsw_sets()) == (2, 1, 2, 1)
    assert libs["two"].xsw_sweeps() == libs["copy"].xsw_sweeps() and libs["two"].xsw_sweeps() % 2 == 0
    assert libs["two_odd"].xsw_sweeps() == libs["copy_odd"].xsw_sweeps() == 49
    return libs


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def grasp32(golden_rollout):
    """32 states of the grasp fixture with the pads loaded (4 envs x 8 instants), half of them with two arm joints pushed into
    their limit windows (slot 3, as tests/test_coop.py does), and 20 actions per env from the fixture's own script"""
    g = golden_rollout
    S = np.concatenate([g["grasp_states"][t] for t in range(23, 31)]).astype(np.float64)
    assert S.shape == (E, 54)
    held = np.abs(S[:, 42:50]).max(axis=1) > 0.1       # three of the fixture's four envs hold the object between the pads
    assert held.sum() == 24 and held[1::2].sum() >= 8 and held[0::2].sum() >= 8
    S[1::2, 1] = 2.0      # joint 2 within 0.2 rad of its upper limit 2.0944
    S[1::2, 3] = -0.1     # joint 4 near its lower limit -0.19198
    A = np.stack([np.concatenate([g["grasp_actions"][(t + k) % 36] for t in range(23, 31)]) for k in range(STEPS)]).astype(np.float64)
    assert A.shape == (STEPS, E, 4)
    return S, A


def _run(lib, f32, S, A):
    """one reset of a copy of the states, and 20 steps from the states themselves: every state visited"""
    out = []
    r = np.array(S, copy=True)
    lib.xsw_coop_reset(C.c_int(f32), C.c_uint64(1), C.c_int64(E), _p(r))
    out.append(r)
    st = np.array(S, copy=True)
    for k in range(STEPS):
        a = np.ascontiguousarray(A[k])
        lib.xsw_coop_step(C.c_int(f32), C.c_uint64(1), C.c_int64(E), _p(st), _p(a))
        out.append(st.copy())
    return np.stack(out)


@pytest.fixture(scope="module")
def runs(builds, grasp32):
    """every build in both precisions, computed once and side by side (the C calls release the interpreter lock)"""
    S, A = grasp32
    keys = [(n, f32) for n in JOBS for f32 in (1, 0)]
    with ThreadPoolExecutor(len(keys)) as ex:
        return dict(zip(keys, ex.map(lambda k: _run(builds[k[0]], k[1], S, A), keys)))


@pytest.mark.parametrize("f32", [1, 0], ids=["float32", "float64"])
@pytest.mark.parametrize("pair", [("two", "copy"), ("two_odd", "copy_odd")], ids=["even_sweeps", "odd_sweeps"])
def test_two_set_sweep_equals_the_copy_form_bit_for_bit(runs, grasp32, f32, pair):
    S, _ = grasp32
    a, b = runs[(pair[0], f32)], runs[(pair[1], f32)]
    assert np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # the comparison saw pad rows at work (the pads still load the object in envs left as they were, after the first steps) ...
    assert (np.abs(a[1:4, 0::2, 42:50]).max(axis=(0, 2)) > 0.1).any()
    # ... and arm-limit rows, in envs that also hold the object: the pushed joints start inside their limit windows
    assert (S[1::2, 1] > 2.0944 - 0.2).all() and (S[1::2, 3] < -0.19198 + 0.2).all()


@pytest.mark.parametrize("f32", [1, 0], ids=["float32", "float64"])
def test_odd_sweep_count_differs_from_the_product(runs, f32):
    """the odd build really runs another number of sweeps (the comparison above is not two copies of one library)"""
    assert not np.array_equal(runs[("two", f32)], runs[("two_odd", f32)])
