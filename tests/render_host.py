"""ctypes view of tests/hostbuild_render (g++ build of csrc/xarm_render_core.h) - CPU-side render tests only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "hostbuild_render")
KIND = {"pick_and_place": 0, "reach": 1, "handover": 2, "stack_tower": 3}
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    from gym_xarm_amd import _native
    so = os.path.join(DIR, "librender_host.so")
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_render_header.py")], stdout=subprocess.DEVNULL)
    srcs = [os.path.join(DIR, "render_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + [
        os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    L = C.CDLL(so)
    cp = C.POINTER(_native.XarmCamera)
    L.rh_default_camera.argtypes = [C.c_int, cp]
    L.rh_make_camera.argtypes = [cp, C.c_void_p]
    L.rh_scene.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    L.rh_render.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64, cp, C.c_void_p, C.c_int32,
                            C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = L
    return L


def camera(kind, **over):
    """the env kind's default xarm_camera (host build of rc_default_camera) with fields overridden"""
    from gym_xarm_amd import _native
    c = _native.XarmCamera()
    assert lib().rh_default_camera(KIND[kind], C.byref(c)) == 0
    for k, v in over.items():
        if k == "target":
            c.target[:] = list(v)
        else:
            setattr(c, k, v)
    return c


def render(kind, rows, cam, num_obj=1, use_stand=False, ids=None):
    """rows: state rows [E, state_dim]; returns rgba uint8 [n, H, W, 4], depth float32 [n, H, W], seg uint8 [n, H, W]"""
    soa = np.ascontiguousarray(np.asarray(rows, dtype=np.float32).T)
    E = soa.shape[1]
    idv = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    n = E if ids is None else len(idv)
    H, W = cam.height, cam.width
    rgba = np.zeros((n, H, W), dtype=np.uint32)
    depth = np.zeros((n, H, W), dtype=np.float32)
    seg = np.zeros((n, H, W), dtype=np.uint8)
    rc = lib().rh_render(KIND[kind], num_obj, int(use_stand), soa.ctypes.data, E, E, C.byref(cam),
                         None if idv is None else idv.ctypes.data, n, rgba.ctypes.data, depth.ctypes.data, seg.ctypes.data)
    assert rc == 0, "invalid camera"
    return rgba.view(np.uint8).reshape(n, H, W, 4), depth, seg


def ref_camera(cam):
    """the NumPy checker's Camera for an xarm_camera"""
    import render_ref as R
    return R.Camera(list(cam.target), cam.distance, cam.yaw_deg, cam.pitch_deg, cam.roll_deg, cam.fov_deg, cam.width, cam.height,
                    cam.near_z, cam.far_z, bool(cam.flags & 1))
