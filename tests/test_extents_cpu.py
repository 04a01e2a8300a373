"""The free list of a reserved arena (lime_amd/csrc/lime_extents.h: first fit over offset-sorted extents, 2 MB granules, merge on return) is host-only
bookkeeping: tests/extents_check.cpp -- a program of its own, built here with g++ under the address and undefined-behaviour sanitizers, no HIP --
checks first fit, rounding, exact fits, the three merges, and a seeded random walk against a brute-force bitmap."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extent_list_first_fit_rounding_and_merging(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ is needed to build tests/extents_check.cpp")
    exe = str(tmp_path / "extents_check")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "lime_amd", "csrc"), os.path.join(ROOT, "tests", "extents_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
