"""The host arithmetic of the LDS aggregation (csrc/knn_agg_plan.h: the form of pass 1, capacities, threads, LDS bytes, the
redo launch; the bitmap's word / bit / slot functions) against its rules and a brute-force grouping:
tests/host/knn_agg_plan_check.cpp, compiled with the host's C++ compiler under the address and undefined-behaviour
sanitizers and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_check_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "knn_agg_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "locations-recommender_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "knn_agg_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "cases pass" in run.stdout
