"""ctypes view of tests/hostbuild_render_views (g++ build of the view code of csrc/xarm_render_core.h) - CPU-side tests only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

import render_host as RH

ROOT = RH.ROOT
DIR = os.path.join(ROOT, "tests", "hostbuild_render_views")
KIND = dict(RH.KIND, rearrange=4)
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    from gym_xarm_amd import _native
    so = os.path.join(DIR, "librender_views_host.so")
    csrc = os.path.join(ROOT, "gym_xarm_amd", "csrc")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_render_header.py")], stdout=subprocess.DEVNULL)
    srcs = [os.path.join(DIR, "render_views_host.cpp"), os.path.join(ROOT, "include", "xarm_hip.h")] + [
        os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, srcs[0]])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.rvh_view_from_camera.argtypes = [C.POINTER(_native.XarmCamera), vp]
    L.rvh_default_view.argtypes = [C.c_int, C.c_int, vp]
    L.rvh_make_view.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int64, C.c_int64, vp, C.c_int, C.c_int, vp]
    L.rvh_render_views.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.c_int64, C.c_int64, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                   C.c_int32, vp, C.c_int32, vp, vp, vp]
    _lib = L
    return L


def view_from_camera(cam):
    """float32 [16]: the host core's rc_view_from_camera of an xarm_camera"""
    v = np.zeros(16, dtype=np.float32)
    assert lib().rvh_view_from_camera(C.byref(cam), v.ctypes.data) == 0, "invalid camera"
    return v


def default_view(kind, which):
    """float32 [16]: rc_default_view (which: 0 world, 1 wrist0, 2 wrist1), or None where the core refuses"""
    v = np.zeros(16, dtype=np.float32)
    return v if lib().rvh_default_view(KIND[kind], which, v.ctypes.data) == 0 else None


def make_view(kind, rows, e, view, W, H, num_obj=1):
    """(eye, fwd, right, up) float32 [4, 3] of rc_make_view for env e of the state rows, or None for an invalid view"""
    soa = np.ascontiguousarray(np.asarray(rows, dtype=np.float32).T)
    v = np.ascontiguousarray(view, dtype=np.float32)
    out = np.zeros(12, dtype=np.float32)
    rc = lib().rvh_make_view(KIND[kind], num_obj, 0, soa.ctypes.data, soa.shape[1], e, v.ctypes.data, W, H, out.ctypes.data)
    assert rc >= 0
    return out.reshape(4, 3) if rc == 1 else None


def render(kind, rows, views, W, H, num_obj=1, use_stand=False, ids=None, flags=0):
    """rows: state rows [E, state_dim]; views float32 [V, 16] (shared) or [n, V, 16] (per position in the id list);
    returns rgba uint8 [n, V, H, W, 4], depth float32 [n, V, H, W], seg uint8 [n, V, H, W]"""
    soa = np.ascontiguousarray(np.asarray(rows, dtype=np.float32).T)
    E = soa.shape[1]
    idv = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
    n = E if ids is None else len(idv)
    vw = np.ascontiguousarray(views, dtype=np.float32)
    per_env = int(vw.ndim == 3)
    assert vw.shape[-1] == 16 and (not per_env or vw.shape[0] == n)
    V = vw.shape[-2]
    rgba = np.zeros((n, V, H, W), dtype=np.uint32)
    depth = np.zeros((n, V, H, W), dtype=np.float32)
    seg = np.zeros((n, V, H, W), dtype=np.uint8)
    rc = lib().rvh_render_views(KIND[kind], num_obj, int(use_stand), soa.ctypes.data, E, E, vw.ctypes.data, V, per_env, W, H, flags,
                                None if idv is None else idv.ctypes.data, n, rgba.ctypes.data, depth.ctypes.data, seg.ctypes.data)
    assert rc == 0
    return rgba.view(np.uint8).reshape(n, V, H, W, 4), depth, seg
