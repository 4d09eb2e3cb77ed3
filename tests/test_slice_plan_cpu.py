"""The launch shape of a few-block inversion (csrc/commit_plan.h slice_plan):
slice_plan_check.cpp is compiled with the host compiler under AddressSanitizer
and UBSan and run as a child process (a stand-alone program: nothing is
preloaded).  It covers full grids (both numbers 1), 1 / 2 / 8 and more blocks,
R of 1 / 2 / 8, blocks of 1 .. 8192 documents around the group (48) and the
minimum slice (192), NC of 0 .. 100 000 around the row scan's 16 384-column
round, several CU counts and both test knobs (forced values below, at and above
their clamps, malformed strings), and checks for every case that the slices'
document ranges cover each block exactly once on group boundaries, that no
slice is empty unless forced, that the grid stays under its cap and that the
row parts cover the columns once within their bounds."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "tf-idf-distributed-system_amd", "csrc")


def test_slice_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "slice_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "slice_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) >= 100000
