"""The two forms of the per-substep pad setup of the cooperative core (csrc/xarm_coop_core.h pad_columns and the head of sweep_all): the
first form (-DXC_PAD_SETUP_V1: a division per pad row for the reciprocal of its diagonal, taken from lane r of column r; the pad columns
scaled by the receiving rows' 1 / d at the head of sweep_all) against the product (every lane's own diagonal from its own M^-1 J^T,
one division for all pad rows; the columns scaled where pad_columns makes them).  Same arithmetic in the same order, so the two host
builds must agree BIT FOR BIT, in float32 and float64, at the product's sweep count and at an odd one, plain, with every row set forced
(-DXC_FORCE_FULL: the arm-limit columns of the pad rows) and with every pad forced live (-DXC_FORCE_PADW: columns of pads that are
not active - their reciprocal diagonal must stay zero).  Modelled on tests/test_sweep_pad_forms.py, same host translation unit."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostbuild", "xarm_sweep_host.cpp")
E, STEPS = 32, 20

# *_full: -DXC_FORCE_FULL, the core's test hook that gives every substep of every env both row sets and all four pads.  On the host an env
# is alone in its row set, and the envs whose joints are pushed into their limit windows let go of the object, so only these builds
# run the instantiation with pad AND arm-limit rows on loaded pads.
JOBS = {"new": [], "v1": ["-DXC_PAD_SETUP_V1"], "new_odd": ["-DXC_SWEEP_ITERS=49"], "v1_odd": ["-DXC_PAD_SETUP_V1", "-DXC_SWEEP_ITERS=49"],
        "new_full": ["-DXC_FORCE_FULL"], "v1_full": ["-DXC_PAD_SETUP_V1", "-DXC_FORCE_FULL"],
        "new_full_odd": ["-DXC_FORCE_FULL", "-DXC_SWEEP_ITERS=49"], "v1_full_odd": ["-DXC_PAD_SETUP_V1", "-DXC_FORCE_FULL", "-DXC_SWEEP_ITERS=49"],
        # *_padw: -DXC_FORCE_PADW, the hook that makes every pad live wherever pad rows are present: the columns of pads that are not
        # active are formed too, and the rows of such a pad keep a zero reciprocal diagonal in both forms
        "new_padw": ["-DXC_FORCE_PADW"], "v1_padw": ["-DXC_PAD_SETUP_V1", "-DXC_FORCE_PADW"],
        "new_padw_odd": ["-DXC_FORCE_PADW", "-DXC_SWEEP_ITERS=49"], "v1_padw_odd": ["-DXC_PAD_SETUP_V1", "-DXC_FORCE_PADW", "-DXC_SWEEP_ITERS=49"]}


def _build(name):
    """tests/hostbuild/libxarm_padsetup_<name>.so, rebuilt when a source is newer"""
    so = os.path.join(os.path.dirname(SRC), "libxarm_padsetup_%s.so" % name)
    srcs = [SRC] + [os.path.join(ROOT, "gym_xarm_amd", "csrc", f) for f in ("xarm_core.h", "xarm7_pd_model.h", "xarm_coop_core.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in srcs):
        subprocess.check_call(["g++", "-Og", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas"] + JOBS[name] + ["-o", so, SRC])
    return so, C.CDLL(so)


@pytest.fixture(scope="module")
def builds():
    with ThreadPoolExecutor(len(JOBS)) as ex:
        res = dict(zip(JOBS, ex.map(_build, JOBS)))
    libs = {k: v[1] for k, v in res.items()}
    assert libs["new"].xsw_sweeps() == libs["v1"].xsw_sweeps() and libs["new"].xsw_sweeps() % 2 == 0
    assert libs["new_odd"].xsw_sweeps() == libs["v1_odd"].xsw_sweeps() == 49
    assert all(l.xsw_sets() == 2 for l in libs.values())
    assert libs["new_full"].xsw_sweeps() == libs["new"].xsw_sweeps() and libs["new_full_odd"].xsw_sweeps() == libs["v1_full_odd"].xsw_sweeps() == 49
    assert libs["new_padw"].xsw_sweeps() == libs["new"].xsw_sweeps() and libs["new_padw_odd"].xsw_sweeps() == libs["v1_padw_odd"].xsw_sweeps() == 49
    # the macro selects other code: the two builds are not one library twice
    assert open(res["new"][0], "rb").read() != open(res["v1"][0], "rb").read()
    return libs


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def grasp32(golden_rollout):
    """the states and actions of tests/test_sweep_forms.py: 32 states of the grasp fixture with the pads loaded (4 envs x 8 instants),
    half of them with joints 2 and 4 pushed into their limit windows (slot 3), and 20 actions per env from the fixture's own script"""
    g = golden_rollout
    S = np.concatenate([g["grasp_states"][t] for t in range(23, 31)]).astype(np.float64)
    assert S.shape == (E, 54)
    held = np.abs(S[:, 42:50]).max(axis=1) > 0.1
    assert held.sum() == 24 and held[1::2].sum() >= 8 and held[0::2].sum() >= 8
    S[1::2, 1] = 2.0      # joint 2 within 0.2 rad of its upper limit 2.0944
    S[1::2, 3] = -0.1     # joint 4 near its lower limit -0.19198
    A = np.stack([np.concatenate([g["grasp_actions"][(t + k) % 36] for t in range(23, 31)]) for k in range(STEPS)]).astype(np.float64)
    assert A.shape == (STEPS, E, 4)
    return S, A


def _run(lib, f32, S, A):
    """one reset of a copy of the states, and 20 steps from the states themselves"""
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
    S, A = grasp32
    keys = [(n, f32) for n in JOBS for f32 in (1, 0)]
    with ThreadPoolExecutor(len(keys)) as ex:
        return dict(zip(keys, ex.map(lambda k: _run(builds[k[0]], k[1], S, A), keys)))


@pytest.mark.parametrize("f32", [1, 0], ids=["float32", "float64"])
@pytest.mark.parametrize("pair", [("new", "v1"), ("new_odd", "v1_odd"), ("new_full", "v1_full"), ("new_full_odd", "v1_full_odd"),
                                  ("new_padw", "v1_padw"), ("new_padw_odd", "v1_padw_odd")],
                         ids=["even_sweeps", "odd_sweeps", "every_row_set_even", "every_row_set_odd", "every_pad_even", "every_pad_odd"])
def test_product_pad_setup_equals_the_first_form_bit_for_bit(runs, f32, pair):
    a, b = runs[(pair[0], f32)], runs[(pair[1], f32)]
    assert np.isfinite(a).all()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # pad impulses were present in envs left as they were (their own row set: pad rows alone; in the *_full builds: pad + arm-limit rows) ...
    assert (np.abs(a[1:4, 0::2, 42:50]).max(axis=(0, 2)) > 0.1).any()
    # ... all four of them in the even envs, whose joints are not pushed into a limit window: every pad's three columns and diagonals are live
    loaded = (np.abs(a[1:4, 0::2, 42:46]) > 0).sum(axis=2)      # lam_p[0..3]: the normal impulses of the four pads
    assert (loaded == 4).any()


@pytest.mark.parametrize("f32", [1, 0], ids=["float32", "float64"])
def test_odd_sweep_count_differs_from_the_product(runs, f32):
    """the odd build really runs another number of sweeps (the comparison above is not two copies of one library)"""
    assert not np.array_equal(runs[("new", f32)], runs[("new_odd", f32)])
    assert not np.array_equal(runs[("new_full", f32)], runs[("new_full_odd", f32)])
