"""View records without a GPU: the host build of the view code (tests/hostbuild_render_views, g++) against the independent
NumPy checker tests/render_views_ref.py - camera construction, images, the validity rule, the default wrist view - and the ABI."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import render_host as RH
import render_ref as R
import render_views_host as VH
import render_views_ref as VR
from test_render_host import states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "xarm_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
W, H = 48, 40                                                # a partial tile row (40 = 2 * 16 + 8)


def default_views(kind):
    """[1 + narms, 16]: world, wrist0 (, wrist1)"""
    return np.stack([VH.default_view(kind, w) for w in range(VR.NARMS[kind] + 1)])


@pytest.fixture(scope="module")
def fixtures(oracle):
    """(kind, rows, num_obj, views, host images) per states() fixture - rendered once, shared, never modified"""
    out = []
    for kind, rows, nobj in states():
        views = default_views(kind)
        out.append((kind, rows, nobj, views, VH.render(kind, rows, views, W, H, num_obj=nobj)))
    return out


def invalid_records(narms):
    """{clause: record}: one violating record per clause of the validity rule, each a valid world view otherwise"""
    good = VR.record(VR.MOUNT_WORLD, (1.0, -1.0, 0.8), (0.2, 0.0, 0.1), (0.0, 0.0, 1.0), 60.0, 0.1, 100.0)

    def rec(**kw):
        v = good.copy()
        for k, x in kw.items():
            v[int(k[1:])] = x
        return v
    bad = {"eye not finite": rec(f1=np.nan), "target not finite": rec(f4=np.inf), "fov not finite": rec(f9=np.nan),
           "mount not an integer": rec(f12=0.5), "mount out of range": rec(f12=3.0), "mount negative": rec(f12=-1.0),
           "fov zero": rec(f9=0.0), "fov 180": rec(f9=180.0), "near zero": rec(f10=0.0), "far below near": rec(f11=0.05),
           "far too large": rec(f11=2e30), "eye equals target": rec(f3=1.0, f4=-1.0, f5=0.8), "up zero": rec(f6=0.0, f7=0.0, f8=0.0),
           "up parallel to the view direction": rec(f6=-0.8, f7=1.0, f8=-0.7)}
    if narms == 1:
        bad["hand of an arm the scene lacks"] = rec(f12=2.0)
    return good, bad


# ------------------------------------------------------------------------------------------------ camera construction
def test_host_camera_of_world_and_wrist_views_equals_the_checker(fixtures):
    for kind, rows, nobj, views, _ in fixtures:
        for e in range(len(rows)):
            for v in range(len(views)):
                got = VH.make_view(kind, rows, e, views[v], W, H, nobj)
                c = VR.ViewCamera(views[v], kind, rows[e].astype(np.float64), W, H)
                want = np.stack([c.eye, c.f, c.s * c.tx, c.u * c.ty])
                assert got is not None and np.abs(got - want).max() <= 1e-5, (kind, e, v, np.abs(got - want).max())


@pytest.mark.parametrize("kind", list(VH.KIND))
def test_view_from_camera_reproduces_the_camera(kind):
    from gym_xarm_amd import _native
    cam = _native.XarmCamera()
    assert RH.lib().rh_default_camera(VH.KIND[kind], C.byref(cam)) == 0
    want = (C.c_float * 12)()
    assert RH.lib().rh_make_camera(C.byref(cam), want) == 0
    view = VH.view_from_camera(cam)
    assert view[12] == VR.MOUNT_WORLD and view[9] == cam.fov_deg and view[10] == cam.near_z and view[11] == cam.far_z
    assert np.array_equal(view, VH.default_view(kind, 0))
    rows = np.zeros((1, 200), dtype=np.float32)              # a world view reads no state
    got = VH.make_view(kind, rows, 0, view, cam.width, cam.height)
    err = np.abs(got.reshape(-1) - np.array(want[:])).max()
    assert err <= 1e-6, (kind, err)
    cam.fov_deg = 180.0                                      # what xarm_render refuses on these fields is refused here
    assert VH.lib().rvh_view_from_camera(C.byref(cam), np.zeros(16, dtype=np.float32).ctypes.data) == -1


def test_default_views_per_kind():
    scene = json.load(open(os.path.join(ROOT, "gym_xarm_amd", "model", "render_scene.json")))["views"]["wrist"]
    for kind in VH.KIND:
        two = kind in ("handover", "stack_tower", "rearrange")
        for which, mount in ((1, VR.MOUNT_HAND0), (2, VR.MOUNT_HAND1)):
            v = VH.default_view(kind, which)
            if which == 2 and not two:
                assert v is None
                continue
            want = VR.record(mount, scene["eye"], scene["target"], scene["up"], scene["fov"], scene["near"], scene["far"])
            assert np.array_equal(v, want), (kind, which)
        assert VH.default_view(kind, 3) is None and VH.default_view(kind, -1) is None


# ------------------------------------------------------------------------------------------------ images
def test_host_images_match_the_numpy_checker(fixtures):
    for kind, rows, nobj, views, (rgba, depth, seg) in fixtures:
        assert rgba.shape == (len(rows), len(views), H, W, 4)
        VR.assert_matches_checker(kind, rows.astype(np.float64), views, rgba, depth, seg, num_obj=nobj)


def test_shared_per_env_and_single_view_calls_agree(fixtures):
    kind, rows, nobj, views, (rgba, depth, seg) = fixtures[3]                     # Handover: three views
    per = np.tile(views[None], (len(rows), 1, 1))
    for a, b in zip(VH.render(kind, rows, per, W, H, num_obj=nobj), (rgba, depth, seg)):
        assert np.array_equal(a, b)
    for v in range(len(views)):
        for a, b in zip(VH.render(kind, rows, views[v:v + 1], W, H, num_obj=nobj), (rgba, depth, seg)):
            assert np.array_equal(a[:, 0], b[:, v])
    ids = [2, -1, 0, 7]                                                           # bad env ids: the invalid image for every view
    a_rgba, a_depth, a_seg = VH.render(kind, rows, views, W, H, num_obj=nobj, ids=ids)
    assert np.array_equal(a_seg[0], seg[2]) and np.array_equal(a_rgba[2], rgba[0])
    for k in (1, 3):
        assert (a_rgba[k] == 0).all() and (a_depth[k] == 0).all() and (a_seg[k] == 255).all()


# ------------------------------------------------------------------------------------------------ validity
@pytest.mark.parametrize("kind", ["pick_and_place", "handover"])
def test_each_clause_of_the_validity_rule_gives_the_invalid_image(fixtures, kind):
    _, rows, nobj, views, _ = [f for f in fixtures if f[0] == kind][0]
    narms = VR.NARMS[kind]
    good, bad = invalid_records(narms)
    assert VR.valid(good, narms) and all(VR.valid(v, narms) for v in views)
    ref = VH.render(kind, rows[:1], np.stack([good, views[1]]), W, H, num_obj=nobj)
    for why, rec in bad.items():
        assert not VR.valid(rec, narms), why
        assert VH.make_view(kind, rows, 0, rec, W, H, nobj) is None, why
        rgba, depth, seg = VH.render(kind, rows[:1], np.stack([good, rec, views[1]]), W, H, num_obj=nobj)
        assert (rgba[0, 1] == 0).all() and (depth[0, 1] == 0).all() and (seg[0, 1] == 255).all(), why
        for got, want in zip((rgba, depth, seg), ref):                            # the neighbours are unaffected
            assert np.array_equal(got[0, 0], want[0, 0]) and np.array_equal(got[0, 2], want[0, 1]), why
    ok = good.copy()
    ok[13:16] = np.nan                                                            # floats 13-15 are ignored
    assert VR.valid(ok, narms) and np.array_equal(VH.render(kind, rows[:1], ok[None], W, H, num_obj=nobj)[2][0, 0], ref[2][0, 0])


# ------------------------------------------------------------------------------------------------ the default wrist view
def _inside(p, x):
    if p["type"] == R.BOX:
        return bool((np.abs((x - p["c"]) @ p["R"]) <= p["h"]).all())
    if p["type"] == R.SPHERE:
        return bool(np.linalg.norm(x - p["c"]) <= p["r"])
    if p["type"] == R.CAPSULE:
        ba = p["b"] - p["a"]
        s = np.clip((x - p["a"]) @ ba / (ba @ ba), 0, 1)
        return bool(np.linalg.norm(x - (p["a"] + s * ba)) <= p["r"])
    return False


def test_default_wrist_view_sees_its_gripper_and_the_scene(fixtures):
    for kind, rows, nobj, views, (rgba, depth, seg) in fixtures:
        for v in range(1, len(views)):
            own = 3 + 2 * (v - 1)
            for e in range(len(rows)):
                frac = (seg[e, v] == own).mean()
                assert 0.02 < frac < 0.60, (kind, e, v, frac)
                assert (seg[e, v] == 1).any(), (kind, e, v)                       # and the table or the floor
    # PickAndPlace grasp_states: the held object.  The fixture's reset draws the grasp per env (env 0 starts with the object
    # half a metre to the side), so "held" is read from the state: the object centre between the fingers in the checker's hand frame
    rows = np.load(os.path.join(GOLDEN, "pnp_oracle_rollout.npz"))["grasp_states"][30].astype(np.float64)
    _, _, seg = VH.render("pick_and_place", rows, VH.default_view("pick_and_place", 1)[None], W, H)
    held = []
    for e in range(len(rows)):
        Rh, ph = R.arm_frames("pick_and_place", rows[e][0:9], 0)[1]
        o = Rh.T @ (rows[e][18:21] - ph)
        held.append(bool(abs(o[0]) < 0.02 and abs(o[1]) < 0.02 and 0.06 < o[2] < 0.15))
    assert sum(held) >= 2 and all((seg[e, 0] == 8).mean() > 0.02 for e in range(len(rows)) if held[e])


def test_default_wrist_eye_is_outside_its_arm_at_every_finger_opening(oracle):
    """the eye lies inside no primitive of its own arm and the rays through the image centre hit none, fingers at 0.01 - 0.04"""
    for kind, rows, nobj in states():
        if kind == "reach":
            widths = [None]                                                       # one gripper box, no finger joints
        else:
            widths = [0.01, 0.02, 0.03, 0.04]
        lay = R.LAYOUT["handover2" if kind == "handover" and nobj == 2 else kind]
        for arm in range(lay["narms"]):
            view = VH.default_view(kind, 1 + arm)
            for wd in widths:
                row = rows[0].astype(np.float64).copy()
                if wd is not None:
                    row[lay["q"] + 9 * arm + 7: lay["q"] + 9 * arm + 9] = wd
                cam = VR.ViewCamera(view, kind, row, W, H)
                prims = [p for p in R.scene(kind, row, num_obj=nobj) if p["seg"] in (2 + 2 * arm, 3 + 2 * arm)]
                assert len(prims) == (8 if kind == "reach" else 10)
                assert not any(_inside(p, cam.eye) for p in prims), (kind, arm, wd)
                _, _, seg = VH.render(kind, row[None], view[None], W, H, num_obj=nobj)
                centre = seg[0, 0, H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1]
                assert not np.isin(centre, (2 + 2 * arm, 3 + 2 * arm)).any(), (kind, arm, wd, centre)


def test_wrist_camera_follows_the_hand(oracle):
    """moving only the seven arm joints leaves the gripper's mask in the wrist image where it was and moves the table"""
    kind = "pick_and_place"
    rows = np.load(os.path.join(GOLDEN, "pnp_oracle_rollout.npz"))["rand_states"][5][:16]
    moved = rows.copy()
    moved[:, 0:7] += np.array([0.25, -0.12, 0.1, 0.15, -0.1, 0.12, 0.3], dtype=moved.dtype)

    def clear(row):                                          # nothing can come between the eye and the gripper: the object is
        Rh, ph = R.arm_frames(kind, row[0:9].astype(np.float64), 0)[1]   # away from the hand and the hand is above the table
        return np.linalg.norm(row[18:21] - ph) > 0.25 and ph[2] > 0.15
    envs = [e for e in range(len(rows)) if clear(rows[e]) and clear(moved[e])][:4]
    assert len(envs) >= 2
    view = VH.default_view(kind, 1)[None]
    _, depth, seg = VH.render(kind, rows[envs], view, W, H)
    _, depth2, seg2 = VH.render(kind, moved[envs], view, W, H)
    for e in range(len(envs)):
        same = ((seg[e, 0] == 3) == (seg2[e, 0] == 3)).mean()
        assert same >= 0.995, (e, same)
        table = (seg[e, 0] == 1) & (seg2[e, 0] == 1)
        assert table.sum() > 50 and np.abs(depth[e, 0][table] - depth2[e, 0][table]).mean() > 1e-3, e


# ------------------------------------------------------------------------------------------------ ABI
def test_header_binding_and_constants_agree():
    from gym_xarm_amd import _native
    src = open(HDR).read()
    assert "#define XARM_VIEW_FLOATS %d" % _native.VIEW_FLOATS in src and _native.VIEW_FLOATS == 16
    assert "#define XARM_RENDER_MAX_VIEWS %d" % _native.RENDER_MAX_VIEWS in src
    for name, val in (("WORLD", VR.MOUNT_WORLD), ("HAND0", VR.MOUNT_HAND0), ("HAND1", VR.MOUNT_HAND1)):
        assert "#define XARM_MOUNT_%s %d" % (name, val) in src
    assert _native.MOUNTS == {"world": 0, "hand0": 1, "hand1": 2}
    for fn in ("xarm_view_from_camera", "xarm_default_view", "xarm_render_views"):
        assert fn in _native.EXPORTS and re.search(r"\bint %s\(" % fn, src)
    assert C.sizeof(_native.XarmCamera) == 52 and C.sizeof(_native.XarmConfig) == 72
    # the rule is stated in the header, the core and the checker
    core = open(os.path.join(ROOT, "gym_xarm_amd", "csrc", "xarm_render_core.h")).read()
    for text in (src, core, VR.valid.__doc__):
        flat = " ".join(text.replace("*", " ").replace("//", " ").split())
        for clause in ("0 < near_z < far_z < 1e30", "|target - eye| > 1e-6", "|up| > 1e-6", "|f x up / |up|| > 1e-6"):
            assert clause.replace("_z", "") in flat.replace("_z", ""), clause


def test_library_exports_the_view_entries():
    from gym_xarm_amd import _native, build
    L = C.CDLL(build.build(verbose=False))
    L.xarm_render_views.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 5 + [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    assert L.xarm_render_views(None, None, 1, 0, 8, 8, 0, None, 1, None, None, None, None) == -1
    L.xarm_default_view.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    assert L.xarm_default_view(None, 0, None) == -1
    # the host helper needs no device: the library's record equals the host build's
    N = _native.load()
    cam = RH.camera("handover")
    v = (C.c_float * 16)()
    assert N.xarm_view_from_camera(C.byref(cam), v) == 0 and np.array_equal(np.array(v[:], dtype=np.float32), VH.view_from_camera(cam))
    cam.near_z = 0.0
    assert N.xarm_view_from_camera(C.byref(cam), v) == -1 and N.xarm_view_from_camera(None, v) == -1
