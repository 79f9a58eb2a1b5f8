"""The flat model table (gym_xarm_amd/model/xarm7_pd.json) against the reference URDF and env file (their numbers, read
from the reference by tools/gen_golden.py into tests/golden/model_reference.json), and the generated kernel header
against the table."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = json.load(open(os.path.join(ROOT, "gym_xarm_amd", "model", "xarm7_pd.json")))
REF = json.load(open(os.path.join(ROOT, "tests", "golden", "model_reference.json")))


def test_generated_header_is_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_model_header.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_links_match_urdf():
    urdf = REF["xarm7_pd_urdf"]
    joints, inertials = urdf["joints"], urdf["inertials"]
    names = [l["name"] for l in JS["links"]]
    for i, l in enumerate(JS["links"]):
        j = joints[l["name"]]
        assert j["type"] == l["joint"]
        assert j["parent"] == ("link_base" if l["parent"] < 0 else names[l["parent"]])
        np.testing.assert_allclose(j["origin_xyz"], l["origin_xyz"], atol=0)
        np.testing.assert_allclose(j["origin_rpy"], l["origin_rpy"], atol=0)
        if l["joint"] != "fixed":
            np.testing.assert_allclose(j["axis"], l["axis"], atol=0)
            assert j["lower"] == l["lower"] and j["upper"] == l["upper"]
            assert (j["damping"] if j["damping"] is not None else 0.0) == l["damping"]
        inert = inertials[l["name"]]
        if inert is None:
            assert l["name"] == "link_eef" and l["mass"] == 1.0 and l["inertia"] == [1.0, 0, 0, 1.0, 0, 1.0]
            continue
        assert inert["mass"] == l["mass"]
        np.testing.assert_allclose(inert["com"], l["com"], atol=0)
        np.testing.assert_allclose(inert["inertia"], l["inertia"], atol=0)
    # Bullet joint indices used by the reference (:31-36): eef 8, hand 9, fingers 10/11
    assert names.index("link_eef") + 1 == 8 and names.index("panda_hand") + 1 == 9
    assert names.index("panda_leftfinger") + 1 == 10 and names.index("panda_rightfinger") + 1 == 11


def test_scene_constants_match_env_file():
    ref = REF["pick_and_place"]
    p = JS["pick_and_place"]
    assert abs(p["time_step"] - 1.0 / 60) < 1e-15 and ref["time_step"] == 1.0 / 60
    for k in ("n_substeps", "distance_threshold", "max_vel", "max_gripper_vel", "max_episode_steps", "pos_low", "pos_high",
              "goal_low", "goal_high", "obj_low", "obj_high", "gripper_low", "gripper_high", "start_gripper_pos"):
        assert p[k] == ref[k], k
    assert p["action_dt"] == p["time_step"] * p["n_substeps"]          # self.dt (:28)
    assert ref["obj_half"] == [0.025, 0.025, 0.04] and p["obj_half"] == [0.025, 0.025, 0.04]
    assert ref["obj_mass"] == 0.5 and p["obj_mass"] == 0.5
    assert ref["finger_motor_force"] == 1000.0 and p["finger_motor_force"] == 1000.0
    assert (ref["gear_ratio"], ref["gear_erp"], ref["gear_max_force"]) == (-1.0, 0.1, 50.0)
    assert JS["solver"]["gear_erp"] == 0.1 and JS["solver"]["gear_max_force"] == 50.0
    assert ref["finger_lateral_friction_grasp"] == 100.0 and JS["solver"]["mu_finger_grasp"] == 100.0


def test_primitives_urdf_round_trips_the_model_table():
    """tools/emit_primitives_urdf.py: the URDF a PyBullet side-by-side run would load carries exactly the model table's
    joints, masses, inertias and the build's collision primitives"""
    import json
    import sys
    import xml.etree.ElementTree as ET
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from emit_primitives_urdf import emit
    js = json.load(open(os.path.join(ROOT, "gym_xarm_amd", "model", "xarm7_pd.json")))
    root = ET.fromstring(emit(js))
    links = {l.attrib["name"]: l for l in root.findall("link")}
    joints = {j.find("child").attrib["link"]: j for j in root.findall("joint")}
    assert len(links) == len(js["links"]) + 1 and len(joints) == len(js["links"])
    for i, l in enumerate(js["links"]):
        e, j = links[l["name"]], joints[l["name"]]
        assert float(e.find("inertial/mass").attrib["value"]) == l["mass"]
        assert [float(x) for x in e.find("inertial/origin").attrib["xyz"].split()] == [float(x) for x in l["com"]]
        assert float(e.find("inertial/inertia").attrib["ixx"]) == l["inertia"][0] and float(e.find("inertial/inertia").attrib["izz"]) == l["inertia"][5]
        assert j.attrib["type"] == l["joint"]
        assert [float(x) for x in j.find("origin").attrib["xyz"].split()] == [float(x) for x in l["origin_xyz"]]
        if l["joint"] != "fixed":
            assert [float(x) for x in j.find("axis").attrib["xyz"].split()] == [float(x) for x in l["axis"]]
            assert float(j.find("limit").attrib["lower"]) == l["lower"] and float(j.find("dynamics").attrib["damping"]) == l["damping"]
        n_col = len(e.findall("collision"))
        assert n_col == (len(js["pads"]["centers_left"]) if i in js["finger_links"] else 0)     # only the pad spheres collide


def test_pybullet_harness_reports_unavailable_cleanly():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "pybullet_harness.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    assert out.stdout.startswith("reference: unavailable (pybullet not importable") or out.stdout.startswith("reference: pybullet")
