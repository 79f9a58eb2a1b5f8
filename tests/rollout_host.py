"""ctypes view of tests/hostbuild_rollout (g++ build of csrc/xarm_rollout_core.h) - CPU-side tests only."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "hostbuild_rollout")
PERM_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 81925)
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(DIR, "librollout_host.so")
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    srcs = [os.path.join(DIR, "rollout_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + [
        os.path.join(csrc, f) for f in ("xarm_rollout_core.h", "xarm_core.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        # -ffp-contract=off: the flag of the device unit (gym_xarm_amd/build.py UNIT_FLAGS)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.rh_perm_bits.argtypes = [C.c_int64]
    L.rh_perm_fill.argtypes = [vp, C.c_int32, C.c_int64, C.c_uint64, vp]
    _lib = L
    return L


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def perm_fill(n_epochs, N, seed, calls):
    """(perm int32 [n_epochs, N] drawn at counter value `calls`, the counter after the call)"""
    perm = np.full((n_epochs, N), -1, np.int32)
    c = np.array([calls], np.int64)
    assert lib().rh_perm_fill(_p(perm), n_epochs, N, seed, _p(c)) == 0
    return perm, int(c[0])


def bits(a):
    return np.ascontiguousarray(a).tobytes()
