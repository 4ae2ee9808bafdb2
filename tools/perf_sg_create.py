#!/usr/bin/env python3
"""Creating a stochastic graph from an edge list that is resident on the device, at cfg3 size (synth.sg_dataset(),
about 5 M edges): the two ways to a servable handle, alternated in one process after one warm-up create of each.

  (a) host build    copy the three columns to the host, then locrec_sg_create (SgGraph)
  (b) device build  locrec_sg_create_from_device (SgGraph.from_device)

Seven repetitions of each: min / median / max of the whole call (host clock, the device idle before and after), and
the HIP-event split of (b) into its phases (locrec_sg_create_from_device_stats).  For the GPU box; run under a timeout.
PERF_SG_PERSONS / PERF_SG_PLACES select another size.

--host-variants: the earlier measurement of this tool instead - locrec_sg_create alone from host arrays: id table vs
sort (LOCREC_SG_NO_DENSE_IDS), with and without the weight dictionary (LOCREC_SG_NO_DICT)."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
import numpy as np  # noqa: E402
import torch  # noqa: E402
from locations_recommender_amd import synth  # noqa: E402



def host_variants():
    g = synth.sg_dataset(seed=0x5EED0003)
    for label, env in (("id table", None), ("sort + bisection", "1"), ("id table", None), ("id table, fp64 weights streamed", "nodict"),
                       ("id table", None)):
        os.environ.pop("LOCREC_SG_NO_DENSE_IDS", None)
        os.environ.pop("LOCREC_SG_NO_DICT", None)
        if env == "nodict":
            os.environ["LOCREC_SG_NO_DICT"] = "1"
        elif env:
            os.environ["LOCREC_SG_NO_DENSE_IDS"] = env
        t0 = time.perf_counter()
        h = pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"])
        dt = time.perf_counter() - t0
        print(f"locrec_sg_create, {h.info()['edges']} edges, {label}: {dt * 1e3:.1f} ms", flush=True)
        h.close()


if "--host-variants" in sys.argv[1:]:
    host_variants()
    sys.exit(0)

REPS = 7
g = synth.sg_dataset(n_persons=int(os.environ.get("PERF_SG_PERSONS", "280000")), n_places=int(os.environ.get("PERF_SG_PLACES", "10000")))
cols = [torch.from_numpy(np.ascontiguousarray(g[k], dt)).cuda()
        for k, dt in (("source_id", np.int64), ("target_id", np.int64), ("balanced_weight", np.float64))]
torch.cuda.synchronize()
print(f"edges {len(cols[0])}, device {torch.cuda.get_device_name(0)}", flush=True)


def host_build():
    s, t, w = (c.cpu().numpy() for c in cols)
    return pkg.SgGraph(s, t, w)


def device_build():
    return pkg.SgGraph.from_device(*cols)


def timed(make):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h = make()
    dt = (time.perf_counter() - t0) * 1e3
    return h, dt


facts = []
for make in (host_build, device_build):       # warm-up: code objects, rocPRIM kernels, the allocator
    h, _ = timed(make)
    facts.append(dict(h.info(), live_count=h.live_count()))
    h.close()
assert facts[0] == facts[1], facts
print("layout facts (both builders):", facts[0], flush=True)

ms = {"host": [], "device": []}
phases = []
for _ in range(REPS):
    h, dt = timed(host_build)
    ms["host"].append(dt)
    h.close()
    h, dt = timed(device_build)
    ms["device"].append(dt)
    phases.append(pkg.SgGraph.device_build_stats())
    h.close()

for label, key in (("(a) device-to-host copy + locrec_sg_create", "host"), ("(b) locrec_sg_create_from_device", "device")):
    v = ms[key]
    print(f"{label}: min {min(v):.2f} ms, median {statistics.median(v):.2f} ms, max {max(v):.2f} ms  ({REPS} repetitions)")
print("(b) by HIP events, median of the repetitions:")
for k, label in (("ranking_ms", "ranking"), ("plan_ms", "live order + plan + maps"), ("scatter_ms", "sorts + scatter + dead slots"),
                 ("dictionary_ms", "dictionary")):
    print(f"    {label}: {statistics.median(p[k] for p in phases):.2f} ms")
med_a, med_b = statistics.median(ms["host"]), statistics.median(ms["device"])
print(f"median (b) / median (a) = {med_b / med_a:.3f}: " + ("the device build is not slower" if med_b <= med_a else "THE DEVICE BUILD IS SLOWER"))
