"""Rendering without a GPU: the camera closed form, the render geometry against the physics model, and the host build of the
render core (tests/hostbuild_render, g++) against the independent NumPy checker tests/render_ref.py."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import render_host as RH
import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "xarm_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")


# ------------------------------------------------------------------------------------------------ camera
@pytest.mark.parametrize("kind", list(R.KINDS))
def test_target_projects_to_the_image_centre(kind):
    cam = R.Camera.default(kind)
    i, j, z = cam.project(cam.target)
    assert abs(i - (cam.height - 1) / 2) < 1e-9 and abs(j - (cam.width - 1) / 2) < 1e-9 and z > 0
    i2, j2, _ = cam.project(cam.target + np.array([0, 0, 0.1]))
    assert i2 < i - 1                                       # a point above the target lands above the centre (row 0 = top)


def test_reference_camera_eyes_equal_the_closed_form():
    # PickAndPlace: target (0.3, 0, 0.2), distance 1.2, yaw 45, pitch -10; Handover: target 0, 1.4, yaw 45, pitch -30
    for kind, tgt, d, yaw, pitch in (("pick_and_place", (0.3, 0, 0.2), 1.2, 45, -10), ("handover", (0, 0, 0), 1.4, 45, -30)):
        y, p = np.radians(yaw), np.radians(pitch)
        want = np.array(tgt) + d * np.array([np.cos(p) * np.sin(y), -np.cos(p) * np.cos(y), -np.sin(p)])
        assert np.allclose(R.Camera.default(kind).eye, want, atol=1e-12)
        c = RH.camera(kind)
        out = (C.c_float * 12)()
        assert RH.lib().rh_make_camera(C.byref(c), out) == 0
        assert np.allclose(np.array(out[:3]), want, atol=1e-6)           # the render core's camera (rc_make_camera)
        assert abs(np.linalg.norm(out[3:6]) - 1) < 1e-6


def test_aspect_and_fov_act_as_expected():
    cam = R.Camera.default("handover")                       # 720 x 480, fov 60 (vertical)
    assert abs(cam.tx / cam.ty - 1.5) < 1e-12 and abs(cam.ty - np.tan(np.radians(30))) < 1e-12
    wide = R.Camera.default("handover", fov=90.0)
    p = cam.target + 0.2 * cam.u
    assert abs(wide.project(p)[0] - (wide.height - 1) / 2) < abs(cam.project(p)[0] - (cam.height - 1) / 2)
    # one pixel subtends the same angle horizontally and vertically (square pixels)
    d = cam.rays().reshape(cam.height, cam.width, 3)
    h = np.linalg.norm(d[240, 361] - d[240, 360])
    v = np.linalg.norm(d[241, 360] - d[240, 360])
    assert abs(h - v) < 1e-12


# ------------------------------------------------------------------------------------------------ geometry
def test_render_geometry_equals_the_physics_dimensions():
    scene = json.load(open(os.path.join(ROOT, "gym_xarm_amd", "model", "render_scene.json")))
    model = json.load(open(os.path.join(ROOT, "gym_xarm_amd", "model", "xarm7_pd.json")))
    assert scene["pick_and_place"]["obj_half"] == model["pick_and_place"]["obj_half"]
    assert scene["stack_tower"]["cube_half"] == model["stack_tower"]["cube_half"]
    for k in ("obj_half", "stand_half", "stand_below_goal", "table_x_min", "table_x_max", "table_half_y", "ground_z"):
        assert scene["handover"][k] == model["handover"][k], k
    assert scene["ground"]["z"] == model["handover"]["ground_z"]
    for k in ("half_x", "half_y", "top_z"):
        assert scene["table"][k] == model["table"][k], k
    assert scene["finger"]["finger_z"] == model["links"][model["finger_links"][0]]["origin_xyz"][2]
    # the generated header is up to date
    import subprocess
    import sys
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_render_header.py"), "--check"],
                          capture_output=True).returncode == 0


def test_hand_and_finger_boxes_equal_the_survey_bboxes():
    scene = json.load(open(os.path.join(ROOT, "gym_xarm_amd", "model", "render_scene.json")))
    assert scene["hand"]["lo"] == [-0.0316, -0.104, -0.026] and scene["hand"]["hi"] == [0.0316, 0.100, 0.066]
    assert scene["finger"]["lo"] == [-0.0105, 0.0, 0.0] and scene["finger"]["hi"] == [0.0105, 0.0264, 0.0539]
    survey = open(os.path.join(ROOT, "SURVEY.md")).read()
    assert "finger hull bbox x∈[−0.0105,0.0105], y∈[0,0.0264], z∈[0,0.0539]" in survey
    assert "hand hull bbox x∈[−0.0316,0.0316], y∈[−0.104,0.100], z∈[−0.026,0.066]" in survey


# ------------------------------------------------------------------------------------------------ host core vs checker
def states():
    """(kind, rows [n, state_dim], num_obj): golden-rollout states of every env kind, StackTower from oracle resets"""
    from oracle import oracle as O
    g = lambda f: np.load(os.path.join(GOLDEN, "%s_oracle_rollout.npz" % f))
    st = O.OracleStackTower(3, seed=1)
    st.reset()
    return [("pick_and_place", g("pnp")["rand_states"][5][:3], 1), ("pick_and_place", g("pnp")["grasp_states"][30][:2], 1),
            ("reach", g("reach")["states"][10][:3], 1), ("handover", g("handover")["states"][20][:3], 1),
            ("handover", g("handover2")["states"][20][:3], 2), ("stack_tower", st.get_state(), 1)]


def assert_matches_checker(kind, rows, rgba, depth, seg, cam, num_obj=1, use_stand=False, seg_frac=0.995):
    """the rule of DESIGN.md 16e: segmentation agrees on >= seg_frac of the pixels and every disagreement lies within 1 px of
    a segmentation boundary of the checker's image; where it agrees, RGB within 2 levels and depth within 1e-4 m (1e-3 m on
    the checker's boundary pixels, where a ray grazes a silhouette and the float32 root is ill-conditioned)"""
    rc = RH.ref_camera(cam)
    for e in range(len(rows)):
        r_rgba, r_depth, r_seg = R.render(kind, rows[e], rc, num_obj=num_obj, use_stand=use_stand)
        agree = seg[e] == r_seg
        bnd = R.boundary(r_seg)
        assert agree.mean() >= seg_frac, (kind, e, agree.mean())
        assert not (~agree & ~bnd).any(), (kind, e, np.argwhere(~agree & ~bnd)[:5])
        dd = np.abs(depth[e].astype(np.float64) - r_depth)
        assert (dd[agree & ~bnd] <= 1e-4).all() and (dd[agree] <= 1e-3).all(), (kind, e, dd[agree].max())
        dc = np.abs(rgba[e].astype(int) - r_rgba.astype(int)).max(-1)
        assert (dc[agree] <= 2).all(), (kind, e, dc[agree].max())
        assert (rgba[e][..., 3] == 255).all()


@pytest.mark.parametrize("size", [(64, 64), (128, 96)])
def test_host_core_matches_the_numpy_checker(oracle, size):
    for kind, rows, nobj in states():
        cam = RH.camera(kind, width=size[0], height=size[1])
        rgba, depth, seg = RH.render(kind, rows, cam, num_obj=nobj)
        assert_matches_checker(kind, rows, rgba, depth, seg, cam, num_obj=nobj)
        assert (seg > 1).any(axis=(1, 2)).all()                  # every image shows the robot


def test_host_core_matches_the_checker_with_shadows_and_the_stand(oracle):
    rows = np.load(os.path.join(GOLDEN, "handover_oracle_rollout.npz"))["states"][10][:2]
    cam = RH.camera("handover", width=96, height=64, flags=1)
    rgba, depth, seg = RH.render("handover", rows, cam, use_stand=True)
    assert_matches_checker("handover", rows, rgba, depth, seg, cam, use_stand=True)
    _, _, seg0 = RH.render("handover", rows, RH.camera("handover", width=96, height=64))
    assert np.array_equal(seg, seg0) or (seg != seg0).mean() < 0.02   # the stand adds a few pixels at most


def test_looking_down_at_the_table_gives_the_plane_distance(oracle):
    """a camera 0.5 m above an empty patch of table, looking (almost) straight down: depth = distance to the plane"""
    rows = np.load(os.path.join(GOLDEN, "pnp_oracle_rollout.npz"))["rand_states"][0][:1]
    cam = RH.camera("pick_and_place", target=(-0.5, 0.3, 0.0), distance=0.5, pitch_deg=-89.0, yaw_deg=0.0, fov_deg=30.0,
                    width=32, height=32)
    rgba, depth, seg = RH.render("pick_and_place", rows, cam)
    assert (seg[0] == 1).all()
    rc = RH.ref_camera(cam)
    D = rc.rays()
    t = (0.0 - rc.eye[2]) / D[:, 2]                          # the table top z = 0 along each ray = its view-axis depth
    assert np.abs(depth[0].reshape(-1) - t).max() < 1e-5


def test_invalid_env_ids_render_zero_images():
    rows = np.load(os.path.join(GOLDEN, "reach_oracle_rollout.npz"))["states"][0][:2]
    cam = RH.camera("reach", width=16, height=8)
    rgba, depth, seg = RH.render("reach", rows, cam, ids=[1, -1, 2, 0])
    for k in (1, 2):
        assert (rgba[k] == 0).all() and (depth[k] == 0).all() and (seg[k] == 255).all()
    ref, _, _ = RH.render("reach", rows, cam)
    assert np.array_equal(rgba[0], ref[1]) and np.array_equal(rgba[3], ref[0])


# ------------------------------------------------------------------------------------------------ ABI
def test_camera_struct_matches_the_header():
    from gym_xarm_amd import _native
    assert C.sizeof(_native.XarmCamera) == 52
    src = open(HDR).read()
    body = src[src.index("typedef struct xarm_camera"):src.index("} xarm_camera;")]
    names = re.findall(r"\b(target|distance|yaw_deg|pitch_deg|roll_deg|fov_deg|near_z|far_z|width|height|flags)\b", body)
    assert names == [f[0] for f in _native.XarmCamera._fields_]
    assert "#define XARM_RENDER_SHADOWS %d" % _native.RENDER_SHADOWS in src
    assert "#define XARM_RENDER_MAX_DIM %d" % _native.RENDER_MAX_DIM in src


def test_library_exports_the_render_entries():
    from gym_xarm_amd import build
    lib = build.build(verbose=False)
    L = C.CDLL(lib)
    assert hasattr(L, "xarm_render") and hasattr(L, "xarm_default_camera")
    L.xarm_render.argtypes = [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 4
    assert L.xarm_render(None, None, None, 1, None, None, None, None) == -1
    L.xarm_default_camera.argtypes = [C.c_void_p, C.c_void_p]
    assert L.xarm_default_camera(None, None) == -1
