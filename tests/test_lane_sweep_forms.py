"""The two forms of the sweep of the one-env-per-lane core (csrc/xarm_core.h xk::substep): one set of impulses with a copy per
row and one loop with a test per arm-limit row (-DXK_SWEEP_V1 -DXK_TABLE_V1, the earlier form) against two sets that the sweeps
read and write in turn, and a loop chosen once per substep with or without arm-limit rows (the product).  Same arithmetic in
the same order, so the two host builds must agree BIT FOR BIT, in float32 and float64, with an even sweep count (the
product's) and with an odd one (the epilogue sweep; the code after the loop then reads the other set)."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostbuild", "xarm_lane_sweep_host.cpp")
E, STEPS = 32, 20
V1 = ["-DXK_SWEEP_V1", "-DXK_TABLE_V1"]
FULL = ["-DXK_SWEEP_FULL"]   # the product form in the full substep too (the product itself runs it in the fast substep alone)
JOBS = {"product": FULL, "v1": V1, "product_odd": FULL + ["-DXK_SWEEP_ITERS=49"], "v1_odd": V1 + ["-DXK_SWEEP_ITERS=49"], "shipped": [], "shipped_odd": ["-DXK_SWEEP_ITERS=49"]}


def _build(name):
    """tests/hostbuild/libxarm_lane_sweep_<name>.so, rebuilt when a source is newer (as conftest.HostCore keeps libxarm_host.so)"""
    so = os.path.join(os.path.dirname(SRC), "libxarm_lane_sweep_%s.so" % name)
    srcs = [SRC] + [os.path.join(ROOT, "gym_xarm_amd", "csrc", f) for f in ("xarm_core.h", "xarm7_pd_model.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs):
        # -Og: a third of the compile time of -O1; the comparison is between builds of the same flags
        subprocess.check_call(["g++", "-Og", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas"] + JOBS[name] + ["-o", so, SRC])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def builds():
    with ThreadPoolExecutor(len(JOBS)) as ex:
        libs = dict(zip(JOBS, ex.map(_build, JOBS)))
    assert [libs[n].xls_sets() for n in JOBS] == [2, 1, 2, 1, 0, 0]
    assert [libs[n].xls_table_v1() for n in JOBS] == [0, 1, 0, 1, 0, 0]
    assert libs["product"].xls_sweeps() == libs["v1"].xls_sweeps() == libs["shipped"].xls_sweeps() and libs["product"].xls_sweeps() % 2 == 0
    assert libs["product_odd"].xls_sweeps() == libs["v1_odd"].xls_sweeps() == libs["shipped_odd"].xls_sweeps() == 49
    return libs


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def grasp32(golden_rollout):
    """32 states of the grasp fixture with the pads loaded (4 envs x 8 instants), half of them with two arm joints pushed into
    their limit windows (as tests/test_sweep_forms.py does), and 20 actions per env from the fixture's own script"""
    g = golden_rollout
    S = np.concatenate([g["grasp_states"][t] for t in range(23, 31)]).astype(np.float64)
    assert S.shape == (E, 54)
    S[1::2, 1] = 2.0      # joint 2 within 0.2 rad of its upper limit 2.0944
    S[1::2, 3] = -0.1     # joint 4 near its lower limit -0.19198
    A = np.stack([np.concatenate([g["grasp_actions"][(t + k) % 36] for t in range(23, 31)]) for k in range(STEPS)]).astype(np.float64)
    assert A.shape == (STEPS, E, 4)
    return S, A


def _run(lib, f32, S, A):
    """one reset of a copy of the states, 20 steps from the states themselves, and beside every step the same step as three
    fast ranges from the same state: (states [1 + STEPS, E, 54], outputs [STEPS, E, out], fast states, fast outputs, fast flags)"""
    od = lib.xls_out_dim()
    r = np.array(S, copy=True)
    lib.xls_reset(C.c_int(f32), C.c_uint64(1), C.c_int64(E), _p(r))
    states, outs, fstates, fouts, oks = [r], [], [], [], []
    st = np.array(S, copy=True)
    for k in range(STEPS):
        a = np.ascontiguousarray(A[k])
        fs, fo, ok = st.copy(), np.zeros((E, od)), np.zeros(E, np.int32)
        lib.xls_step_fast3(C.c_int(f32), C.c_uint64(1), C.c_int64(E), _p(fs), _p(a), _p(fo), ok.ctypes.data_as(C.POINTER(C.c_int)))
        o = np.zeros((E, od))
        lib.xls_step(C.c_int(f32), C.c_uint64(1), C.c_int64(E), _p(st), _p(a), _p(o))
        states.append(st.copy()); outs.append(o); fstates.append(fs); fouts.append(fo); oks.append(ok)
    return np.stack(states), np.stack(outs), np.stack(fstates), np.stack(fouts), np.stack(oks)


@pytest.fixture(scope="module")
def runs(builds, grasp32):
    """every build in both precisions, computed once and side by side (the C calls release the interpreter lock)"""
    S, A = grasp32
    keys = [(n, f32) for n in JOBS for f32 in (1, 0)]
    with ThreadPoolExecutor(len(keys)) as ex:
        return dict(zip(keys, ex.map(lambda k: _run(builds[k[0]], k[1], S, A), keys)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("f32", [1, 0], ids=["float32", "float64"])
@pytest.mark.parametrize("pair", [("product", "v1"), ("product_odd", "v1_odd"), ("shipped", "v1"), ("shipped_odd", "v1_odd")],
                         ids=["even_sweeps", "odd_sweeps", "shipped_even_sweeps", "shipped_odd_sweeps"])
def test_product_sweep_equals_the_first_form_bit_for_bit(builds, runs, grasp32, f32, pair):
    S, _ = grasp32
    a, b = runs[(pair[0], f32)], runs[(pair[1], f32)]
    for x, y in zip(a, b):
        assert np.isfinite(x).all()
        assert np.array_equal(_bits(x), _bits(y))
    # both loops of the product ran.  The pushed envs start every substep of the reset's first tick and of the first step with
    # joints 2 and 4 inside their limit windows: the loop with arm-limit rows ...
    lo, hi, win = np.zeros(7), np.zeros(7), C.c_double()
    builds[pair[0]].xls_limits(_p(lo), _p(hi), C.byref(win))
    inside = (S[:, 0:7] - lo < win.value) | (hi - S[:, 0:7] < win.value)
    assert inside[1::2, 1].all() and inside[1::2, 3].all()
    # ... and the envs left as they were have no arm joint inside a window at the start of the first steps: the limit-free loop
    states = a[0]
    free = ~((states[1:4, 0::2, 0:7] - lo < win.value) | (hi - states[1:4, 0::2, 0:7] < win.value)).any(axis=2)
    assert not inside[0::2].any() and free.any()
    # the comparison saw table rows at work (an object resting on the table carries a normal impulse) and pad rows
    assert (np.abs(states[1:, :, 34:42]).max(axis=2) > 1e-3).any()
    assert (np.abs(states[1:4, :, 42:50]).max(axis=(0, 2)) > 0.1).any()


@pytest.mark.parametrize("f32", [1, 0], ids=["float32", "float64"])
def test_odd_sweep_count_differs_from_the_product(runs, f32):
    """the odd build really runs another number of sweeps (the comparison above is not two copies of one library)"""
    assert not np.array_equal(runs[("product", f32)][0], runs[("product_odd", f32)][0])


@pytest.mark.parametrize("f32", [1, 0], ids=["float32", "float64"])
@pytest.mark.parametrize("name", ["product", "v1", "shipped"])
def test_fast_ranges_equal_the_whole_step_bit_for_bit(runs, name, f32):
    """the fast ranges [0,5), [5,10), [10,15) of a step against the whole step from the same state, on every (step, env) the
    ranges accept and in particular on the envs that are never handed off; the host build gives the two substeps the same bits"""
    states, outs, fstates, fouts, oks = runs[(name, f32)]
    ok = oks.astype(bool)
    never = ok.all(axis=0)
    assert never.any()              # envs that stay on the fast ranges for all 20 steps ...
    assert (~ok).any(axis=0).any()  # ... and envs that were handed off (a pad row was active): the flag is not constant
    assert np.array_equal(_bits(fstates[:, never]), _bits(states[1:, never]))
    assert np.array_equal(_bits(fouts[:, never]), _bits(outs[:, never]))
    assert np.array_equal(_bits(fstates[ok]), _bits(states[1:][ok]))
    assert np.array_equal(_bits(fouts[ok]), _bits(outs[ok]))
