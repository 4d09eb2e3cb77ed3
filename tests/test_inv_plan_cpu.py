"""The host side of an incremental inversion (csrc/commit_plan.h):
inv_plan_check.cpp is compiled with the host compiler under AddressSanitizer
and UBSan and run as a child process (a stand-alone program: nothing is
preloaded).  It checks inversion_plan with each condition flipped one at a
time (full plan, term-major, inv_docs of 0 / 8191 / 8192 / 8193 / > N, the
TFIDF_FULL_INVERSION switch, NC equal and larger), the formula k_blk_remap runs
against a naive rebuild of the offset row for random old and new occupancy
bitmaps with old a subset of new (new slots below the first, between and above
the last old slot, a kept block with total 0, NC_inv = 0, the 32-slot word
edge), and the posting-escape keep bound against a linear filter (empty lists,
an escape exactly at the base)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "tf-idf-distributed-system_amd", "csrc")


def test_inversion_plan_remap_and_escape_bound_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "inv_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(HERE, "inv_plan_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) >= 1000
