"""ctypes view of tests/hostbuild_rearrange (g++ build of the cube core csrc/xarm_stack_core.h for the scene of
csrc/xarm_rearrange_core.h, float64 and float32) - CPU-side tests only.  Rows are float64 state rows [E, 160] in the layout of
the header comment of xarm_stack_core.h with N = 4."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "hostbuild_rearrange")
STATE_DIM, OBS_DIM, GOAL_DIM = 160, 68, 12
# state fields (xra::Rearrange4::K_*)
Q, QD, QT, BP, BQ, BV, BW, GOAL, LT, LP, STEPS, EPISODE = 0, 18, 36, 54, 66, 82, 94, 106, 118, 150, 158, 159
# StackTower's (xs::Tower3::K_*)
S_BP, S_BQ, S_BV, S_BW, S_GOAL, S_LT, S_LP, S_STEPS, S_EPISODE = 54, 63, 75, 84, 93, 102, 126, 134, 135
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "librearrange_host.so")
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    srcs = [os.path.join(DIR, "rearrange_host.cpp"), os.path.join(ROOT, "tests", "hostbuild", "cube_pair_host.h")] + [
        os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-pthread", "-o", tmp, srcs[0]])
        os.replace(tmp, so)
    L = C.CDLL(so)
    vp, i64, u64, i32 = C.c_void_p, C.c_int64, C.c_uint64, C.c_int
    L.ra_dims.argtypes = [vp]
    L.ra_init.argtypes = [i32, u64, i64, i32, i64, vp]
    L.ra_step.argtypes = [i32, u64, i64, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ra_reset.argtypes = [i32, u64, i64, i32, i64, vp, vp, vp, vp, vp, vp]
    L.ra_compute_reward.argtypes = [i32, vp, vp, i64, vp]
    L.ra_class_order.argtypes = [vp, i64, i32, vp]
    _lib = L
    return L


def _p(a):
    return a.ctypes.data


def init(E, f32=0, seed=0, off=0, rt=0):
    st = np.zeros((E, STATE_DIM))
    lib().ra_init(f32, seed, off, rt, E, _p(st))
    return st


def step(state, actions, f32=0, seed=0, off=0, rt=0):
    """-> state, obs, ag, dg, reward, done, success, class key (row-set class of the last substep)"""
    st = np.ascontiguousarray(state, dtype=np.float64).copy()
    E = st.shape[0]
    act = np.ascontiguousarray(actions, dtype=np.float64)
    obs, ag, dg = np.zeros((E, OBS_DIM)), np.zeros((E, GOAL_DIM)), np.zeros((E, GOAL_DIM))
    rew, done, succ, key = np.zeros(E), np.zeros(E, np.uint8), np.zeros(E, np.uint8), np.zeros(E, np.uint8)
    lib().ra_step(f32, seed, off, rt, E, _p(st), _p(act), _p(obs), _p(ag), _p(dg), _p(rew), _p(done), _p(succ), _p(key))
    return st, obs, ag, dg, rew, done, succ, key


def reset(state, mask=None, f32=0, seed=0, off=0, rt=0):
    st = np.ascontiguousarray(state, dtype=np.float64).copy()
    E = st.shape[0]
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    obs, ag, dg, key = np.zeros((E, OBS_DIM)), np.zeros((E, GOAL_DIM)), np.zeros((E, GOAL_DIM)), np.zeros(E, np.uint8)
    lib().ra_reset(f32, seed, off, rt, E, _p(st), None if m is None else _p(m), _p(obs), _p(ag), _p(dg), _p(key))
    return st, obs, ag, dg, key


def compute_reward(ag, g, rt):
    a, b = np.ascontiguousarray(ag, dtype=np.float32).reshape(-1, 12), np.ascontiguousarray(g, dtype=np.float32).reshape(-1, 12)
    out = np.zeros(a.shape[0], np.float32)
    lib().ra_compute_reward(rt, _p(a), _p(b), a.shape[0], _p(out))
    return out


def class_order(key, group=32):
    k = np.ascontiguousarray(key, dtype=np.uint8)
    order = np.zeros(k.size, np.int32)
    r = lib().ra_class_order(_p(k), k.size, group, _p(order))
    assert r >= 0, "not a permutation"
    return order, bool(r)


def live_cubes(parked):
    return [c for c in range(4) if c != parked]


def from_stack(st_rows, parked, park_xy=(0.0, 0.45)):
    """Rearrange rows holding a StackTower state [E, 136]: its three cubes become the Rearrange cubes other than `parked`,
    in order; cube `parked` rests on the table at park_xy, its goal where it lies"""
    s3 = np.asarray(st_rows, dtype=np.float64)
    E = s3.shape[0]
    r = np.zeros((E, STATE_DIM))
    r[:, 0:54] = s3[:, 0:54]
    for j, c in enumerate(live_cubes(parked)):
        r[:, BP + 3 * c:BP + 3 * c + 3] = s3[:, S_BP + 3 * j:S_BP + 3 * j + 3]
        r[:, BQ + 4 * c:BQ + 4 * c + 4] = s3[:, S_BQ + 4 * j:S_BQ + 4 * j + 4]
        r[:, BV + 3 * c:BV + 3 * c + 3] = s3[:, S_BV + 3 * j:S_BV + 3 * j + 3]
        r[:, BW + 3 * c:BW + 3 * c + 3] = s3[:, S_BW + 3 * j:S_BW + 3 * j + 3]
        r[:, GOAL + 3 * c:GOAL + 3 * c + 3] = s3[:, S_GOAL + 3 * j:S_GOAL + 3 * j + 3]
        r[:, LT + 8 * c:LT + 8 * c + 8] = s3[:, S_LT + 8 * j:S_LT + 8 * j + 8]
    r[:, BP + 3 * parked:BP + 3 * parked + 3] = [park_xy[0], park_xy[1], 0.025]
    r[:, BQ + 4 * parked + 3] = 1.0
    r[:, GOAL + 3 * parked:GOAL + 3 * parked + 3] = [park_xy[0], park_xy[1], 0.025]
    r[:, LP:LP + 8] = s3[:, S_LP:S_LP + 8]
    r[:, STEPS], r[:, EPISODE] = s3[:, S_STEPS], s3[:, S_EPISODE]
    return r


def to_stack(rows, parked, like):
    """the StackTower view of Rearrange rows (cube `parked` dropped); `like` supplies the StackTower goals"""
    r = np.asarray(rows, dtype=np.float64)
    s3 = np.array(like, dtype=np.float64, copy=True)
    s3[:, 0:54] = r[:, 0:54]
    for j, c in enumerate(live_cubes(parked)):
        s3[:, S_BP + 3 * j:S_BP + 3 * j + 3] = r[:, BP + 3 * c:BP + 3 * c + 3]
        s3[:, S_BQ + 4 * j:S_BQ + 4 * j + 4] = r[:, BQ + 4 * c:BQ + 4 * c + 4]
        s3[:, S_BV + 3 * j:S_BV + 3 * j + 3] = r[:, BV + 3 * c:BV + 3 * c + 3]
        s3[:, S_BW + 3 * j:S_BW + 3 * j + 3] = r[:, BW + 3 * c:BW + 3 * c + 3]
        s3[:, S_LT + 8 * j:S_LT + 8 * j + 8] = r[:, LT + 8 * c:LT + 8 * c + 8]
    s3[:, S_LP:S_LP + 8] = r[:, LP:LP + 8]
    s3[:, S_STEPS], s3[:, S_EPISODE] = r[:, STEPS], r[:, EPISODE]
    return s3
