"""Row-set census of the cooperative PickAndPlace sweep: builds tests/hostbuild/xarm_row_census.cpp with g++
(the host float32 cooperative core with the XC_ROW_CENSUS counting hook of csrc/xarm_coop_core.h compiled in) and runs it.
CPU only.

  python tools/row_census.py [envs, default 256] [steps, default 150]
  python tools/row_census.py --stages [envs] [steps]     the resets per hand-off stage instead (tests/hostbuild/xarm_stage_census.cpp,
                                                         DESIGN.md 4b "Resets per hand-off stage")
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostbuild", "xarm_row_census.cpp")
STAGE_SRC = os.path.join(ROOT, "tests", "hostbuild", "xarm_stage_census.cpp")


def build(src, exe):
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, src])
    return exe


def main():
    args = sys.argv[1:]
    src = SRC
    if args and args[0] == "--stages":
        src, args = STAGE_SRC, args[1:]
    with tempfile.TemporaryDirectory() as d:
        exe = build(src, os.path.join(d, os.path.splitext(os.path.basename(src))[0]))
        subprocess.check_call([exe] + args[:2])


if __name__ == "__main__":
    main()
