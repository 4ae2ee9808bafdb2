"""The host arithmetic of the stochastic graph's device build (csrc/sg_layout_plan.h: the piece plan from the scan's
totals with its two refusals, the id-table and 16-bit-column rules, radix bits, byte figures, persist_pw) against a
row-by-row walk of the layout and against literals: tests/host/sg_layout_plan_check.cpp, compiled with the host's C++
compiler under the address and undefined-behaviour sanitizers and run as its own program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_plan_check_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "sg_layout_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "locations-recommender_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "sg_layout_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "cases pass" in run.stdout
