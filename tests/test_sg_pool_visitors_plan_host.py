"""The host plan of a pool visitors call (csrc/sg_pool_visitors_plan.h: the members asked, their visitors and gathered CSR,
tiles and stage, the tables' places in the call's buffers, the waves, the emit order) against brute force and literals:
tests/host/sg_pool_visitors_plan_check.cpp, compiled with the host's C++ compiler and run - with the address and
undefined-behaviour sanitizers where the compiler has them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(cxx, exe, extra):
    built = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", *extra, "-I", os.path.join(ROOT, "locations-recommender_amd", "csrc"),
                            os.path.join(ROOT, "tests", "host", "sg_pool_visitors_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    if built.returncode != 0:
        return None
    return subprocess.run([exe], capture_output=True, text=True)


def test_plan_check_program(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    run = _build_and_run(cxx, str(tmp_path / "sg_pool_visitors_plan_check"), [])
    assert run is not None, "the check program does not compile"
    assert run.returncode == 0, run.stderr
    assert "cases pass" in run.stdout
    # once more under the host sanitizers (a stand-alone program: nothing is preloaded); a compiler without them is no failure
    san = _build_and_run(cxx, str(tmp_path / "sg_pool_visitors_plan_check_san"),
                         ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if san is not None:
        assert san.returncode == 0, san.stderr
        assert "cases pass" in san.stdout
