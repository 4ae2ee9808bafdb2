"""The host arithmetic of the batched top-K (csrc/knn_topk_plan.h: the chunk plan of a tiled scan and its merge levels,
the admission of a batch to the head / tail form, knn_side_topk's LDS) against its invariants over a sweep, against tuples
recorded from enqueue_topk before the arithmetic moved, and against brute-force recomputation:
tests/host/knn_topk_plan_check.cpp, compiled with the host's C++ compiler under the address and undefined-behaviour
sanitizers and run as its own program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_check_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "knn_topk_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "locations-recommender_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "knn_topk_plan_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "cases pass" in run.stdout
