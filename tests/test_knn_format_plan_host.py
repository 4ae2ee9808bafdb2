"""The decision that selects a KNN index's format and kernel path (csrc/knn_format_plan.h, shared by both builders) on
both sides of every limit of DESIGN.md's "Numeric limits": tests/host/knn_format_plan_check.cpp, compiled with the host's
C++ compiler under the address and undefined-behaviour sanitizers and run as its own program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_format_plan_check_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "knn_format_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "locations-recommender_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "knn_format_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "cases pass" in run.stdout
