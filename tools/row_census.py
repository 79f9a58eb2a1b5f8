"""Row-set census of the cooperative PickAndPlace sweep: builds tests/hostbuild/xarm_row_census.cpp with g++
(the host float32 cooperative core with the XC_ROW_CENSUS counting hook of csrc/xarm_coop_core.h compiled in) and runs it.
CPU only.

  python tools/row_census.py [envs, default 256] [steps, default 150]
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostbuild", "xarm_row_census.cpp")


def main():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "xarm_row_census")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, SRC])
        subprocess.check_call([exe] + sys.argv[1:3])


if __name__ == "__main__":
    main()
