#!/usr/bin/env python3
"""Times of every region set's place visits from one device-resident table (csrc/region_sets.hip, prep.RegionSetPlan)
beside what a user without it writes: mask = (region == a) | (region == b), then col[mask] for the five columns.

Default: 25 M place-visit rows as CUDA tensors, once with R = 3 regions (6 sets) and once with R = 16 (136 sets),
regions uniform.  Per shape: both forms' results are compared for equality once, one warm-up each, then --repeats
alternated runs of "all sets"; HIP-event and wall-clock (host clock around work that ends in a device synchronise)
medians, min and max; the one partition of the plan is timed on its own and is NOT inside the plan's per-run time.
Host synchronisations per set, counted from the shape of the calls: the plan's gather waits twice - the binding
waits for torch's stream before the call and the library for its own stream at the end, sizes coming from the
offsets already on the host; the mask form's col[mask] has to learn the size of its result on the host, once per
indexed column, which torch does with a device-to-host copy of the count - one per boolean-mask index.
Results go to stdout; keep them as profiles/region_sets_perf.txt."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
prep = pkg.prep
COLUMNS = prep.PLACE_VISIT_COLUMNS


def table(n, n_regions, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    r = lambda lo, hi: torch.randint(lo, hi, (n,), generator=g, device="cuda", dtype=torch.int64)   # noqa: E731
    return {"person_id": r(2040, 2040 + max(2, n // 40)), "timestamp": r(1_600_000_000_000, 1_607_776_000_000),
            "place_id": r(40, 100_040), "region_id": r(0, n_regions) * 7 - 5, "category_id": r(0, 20)}


def masks_all_sets(pv, sets):
    """The parent commit's way: one boolean mask per set, one boolean-mask index per column."""
    region = pv["region_id"]
    syncs = 0
    last = None
    for rs in sets:
        mask = region == rs[0]
        if len(rs) == 2:
            mask = mask | (region == rs[1])
        last = {k: pv[k][mask] for k in COLUMNS}
        syncs += len(COLUMNS)
    return last, syncs


def plan_all_sets(plan, sets):
    last = None
    for rs in sets:
        last = plan.place_visits(rs)
    return last, 2 * len(sets)


def measure(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b), out


def mmm(xs):
    xs = np.asarray(xs, np.float64)
    return f"{np.median(xs):.3f} ({xs.min():.3f} - {xs.max():.3f})"


def shape(n, n_regions, repeats):
    pv = table(n, n_regions, 0x5EED0A00 + n_regions)
    ids = prep.extract_region_ids(pv["region_id"]).tolist()
    sets = prep.region_sets(ids)
    wall_p, ev_p, plan = measure(lambda: prep.RegionSetPlan(pv, ids))
    part = [measure(lambda: prep.RegionSetPlan(pv, ids))[:2] for _ in range(3)]
    for rs in sets[:2] + sets[-2:]:                       # equality of the two forms, outside the timed runs
        got, want = plan.place_visits(rs), masks_all_sets(pv, [rs])[0]
        assert all(torch.equal(got[k], want[k]) for k in COLUMNS), rs
    masks_all_sets(pv, sets)                              # warm-up of both
    plan_all_sets(plan, sets)
    t = {"mask": ([], []), "plan": ([], [])}
    syncs = {}
    for _ in range(repeats):
        for name, fn in (("mask", lambda: masks_all_sets(pv, sets)), ("plan", lambda: plan_all_sets(plan, sets))):
            wall, ev, (_, s) = measure(fn)
            t[name][0].append(wall)
            t[name][1].append(ev)
            syncs[name] = s / len(sets)
    rows_out = sum(plan.count(rs) for rs in sets)
    print(f"R = {n_regions}: {n:,} rows, {len(sets)} sets, {rows_out:,} rows out over all sets; ms, median (min - max) of {repeats} alternated runs")
    print(f"    one partition (not in the plan's runs)   wall {mmm([p[0] for p in part])}   HIP events {mmm([p[1] for p in part])}   first call: wall {wall_p:.3f}")
    for name, what in (("mask", "mask + col[mask] x 5, all sets   "), ("plan", "plan.place_visits, all sets      ")):
        print(f"    {what}        wall {mmm(t[name][0])}   HIP events {mmm(t[name][1])}   host syncs per set {syncs[name]:.0f}")
    print(f"    median mask / median plan: wall {np.median(t['mask'][0]) / np.median(t['plan'][0]):.2f}, "
          f"HIP events {np.median(t['mask'][1]) / np.median(t['plan'][1]):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=25_000_000)
    ap.add_argument("--regions", type=int, nargs="*", default=[3, 16])
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    print(torch.cuda.get_device_name(0))
    for r in a.regions:
        shape(a.rows, r, a.repeats)


if __name__ == "__main__":
    main()
