"""The element order of the head / tail image (csrc/knn_ht_order.h: one routine for the host builder and the device
builder) on literal lane groups, random ones and an exhaustive search of small ones: tests/host/knn_ht_order_check.cpp,
compiled with the host's C++ compiler under the address and undefined-behaviour sanitizers and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_order_check_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "knn_ht_order_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "locations-recommender_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "knn_ht_order_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "cases pass" in run.stdout
