"""Every kernel launch of the offline device steps is checked where it is made: the seven units, and the headers they
share, launch through csrc/offline.h's LOCREC_LAUNCH (launch, then hipGetLastError with the call site's file and line) and
nowhere write hipLaunchKernelGGL themselves.  knn_host_build.h is exempt: a fragment of the scans' translation unit, it
checks its one launch by hand.  So is sg_build_shared.h, which the device build (sg_create_device.hip, one of the units)
calls for the weight dictionary: sg.hip includes it in front of its kernels, where offline.h - which defines kernels -
cannot come, so its one launch is LOCREC_LAUNCH written out."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "locations-recommender_amd", "csrc")
UNITS = ("knn_build.hip", "prep.hip", "dedup.hip", "rank_batch.hip", "region_sets.hip", "sample.hip", "sg_create_device.hip")
SHARED = ("offline.h", "prep_cols.h", "place_grid.h", "knn_build_open.h")


def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_offline_units_launch_through_the_checked_form_only():
    offline = read("offline.h")
    # the helper: one definition, the launch followed at once by the check
    assert len(re.findall(r"#define\s+LOCREC_LAUNCH\b", offline)) == 1
    helper = re.search(r"#define LOCREC_LAUNCH\(.*?while \(0\)", offline, re.S).group(0)
    assert re.search(r"hipLaunchKernelGGL\(kern, grid, block, lds, stream, __VA_ARGS__\);\s*\\\s*"
                     r"LOCREC_HIP_TRY\(hipGetLastError\(\)\);", helper), helper
    assert offline.count("hipLaunchKernelGGL(") == 1, "offline.h launches outside LOCREC_LAUNCH"
    sites = 0
    for name in UNITS + SHARED:
        text = read(name)
        if name != "offline.h":
            assert "hipLaunchKernelGGL(" not in text, f"{name} launches a kernel without LOCREC_LAUNCH"
        for other in ("<<<", "hipLaunchKernel(", "hipExtLaunchKernelGGL(", "hipExtLaunchKernel(", "hipModuleLaunchKernel(",
                      "hipLaunchCooperativeKernel(", "LOCREC_LAUNCH_PROFILED("):
            assert other not in text, f"{name} launches a kernel through {other} instead of LOCREC_LAUNCH"
        # a check written out after a launch is the second style this rule replaces ((void)hipGetLastError() clears a
        # tolerated failure and stays)
        written_out = re.findall(r"LOCREC_HIP_TRY\(hipGetLastError\(\)\)", text)
        assert len(written_out) == (1 if name == "offline.h" else 0), f"{name} checks a launch by hand"
        sites += len(re.findall(r"\bLOCREC_LAUNCH\(", text)) - (1 if name == "offline.h" else 0)
    assert sites > 120, sites
    for name in UNITS:
        assert re.search(r"\bLOCREC_LAUNCH\(", read(name)), f"{name}: no launch seen"
