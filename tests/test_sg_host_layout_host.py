"""The host build's layout of the stochastic graph (csrc/sg_host_layout.h: vertex ranking, live order, piece plan, edge
scatter with the weight interleave and the dead-slot CSR, seg_out / lane_out / lrows, the fused experiment's second piece
list) against a naive model that knows nothing of pieces, over small graphs, three shards of one among them:
tests/host/sg_host_layout_check.cpp, compiled with the host's C++ compiler under the address and undefined-behaviour
sanitizers and run as its own program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_layout_check_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "sg_host_layout_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "locations-recommender_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "sg_host_layout_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "cases pass" in run.stdout
