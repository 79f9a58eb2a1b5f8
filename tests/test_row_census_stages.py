"""tools/row_census.py --stages: the per-hand-off-stage reset census (tests/hostbuild/xarm_stage_census.cpp, DESIGN.md 4b "Resets per
hand-off stage") builds with g++ and its classes add up.  A sanity test of the tool, not of a number."""
import importlib.util
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_census_builds_and_its_classes_add_up(tmp_path):
    spec = importlib.util.spec_from_file_location("row_census", os.path.join(ROOT, "tools", "row_census.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    exe = tool.build(tool.STAGE_SRC, str(tmp_path / "xarm_stage_census"))
    r = subprocess.run([exe, "32", "60"], stdout=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 0
    m = re.search(r"^resets: (\d+) = A (\d+) \+ B0 (\d+) \+ B1 (\d+) \+ B2 (\d+)$", r.stdout, re.M)
    assert m, r.stdout
    n, a, b0, b1, b2 = (int(x) for x in m.groups())
    assert n > 0 and a + b0 + b1 + b2 == n
    # one table row per class, per env and per union of 4, with the class's n
    for name, k in (("A", a), ("B0", b0), ("B1", b1), ("B2", b2)):
        assert re.search(r"^\| %s, per env \| %d \|" % (name, k), r.stdout, re.M), (name, r.stdout)
        assert re.search(r"^\| %s, union of 4 \| %d \|" % (name, (k + 3) // 4), r.stdout, re.M), (name, r.stdout)
