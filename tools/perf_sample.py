#!/usr/bin/env python3
"""Times of the sample generator on the device (csrc/sample.hip, sample.py).

1. The shipped scale (bin/sample_generator.sh of the reference: 3,000,000 persons, 30,000 places): persons, places and
   names once, then --repeats location-visit calls into preallocated-size outputs.  Per call the HIP-event times of the
   count-and-scan phase and of the fill (locrec_sample_location_visits_stats), and bytes written / fill time as a share
   of the HBM STORE BOUND: 6.0 TB/s, the lower end of the plain-store rate MI355X_MICROARCH.md measures (6.0 - 6.2
   TB/s; HBM3E peak 8.0 TB/s by specification).
2. At --small-persons (300,000): the device call alternated with the only route there was before it - the numpy
   restatement (tests/sample_cases.py) plus the upload of its six columns - wall clock around work that ends in a device
   synchronise, --repeats runs each, and the two results compared bit for bit once.
Results go to stdout; keep them as profiles/sample_generator_perf.txt."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import sample_cases as sc  # noqa: E402

pkg = graft.load_package()
sample = pkg.sample
STORE_BOUND_TBS = 6.0


def mmm(xs):
    xs = np.asarray(xs, np.float64)
    return f"{np.median(xs):.3f} ({xs.min():.3f} - {xs.max():.3f})"


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def shipped(d, persons_n, places_n, repeats):
    regions, cats = d["regions"], d["categories"]
    _, min_place, min_person = sample.id_scheme(len(cats), places_n)
    from_ms, hours, days = sample.year_interval(d["year"])
    t_p, persons = wall(lambda: sample.generate_persons(regions, persons_n, min_person, device=True))
    t_pl, places = wall(lambda: sample.generate_places(regions, places_n, min_place, len(cats), device=True))
    t_n, names = wall(lambda: sample.place_names(places["id"], places["category_id"], cats))
    print(f"shipped scale: {len(persons['id']):,} persons {t_p:.3f} ms, {len(places['id']):,} places {t_pl:.3f} ms, "
          f"{len(names[1]):,} name units {t_n:.3f} ms (wall, first call each)")
    total = sample.location_visits_count(persons, regions, from_ms, hours, days)
    for shared in (True, False):
        count_ms, fill_ms, walls = [], [], []
        for _ in range(repeats + 1):                       # (the first run is the warm-up)
            w, v = wall(lambda: sample.generate_location_visits(persons, regions, from_ms, hours, days, shared_factor=shared,
                                                                capacity=total))
            st = sample.location_visits_stats()
            assert st["rows"] == total == len(v["person_id"])
            del v
            count_ms.append(st["count_ms"]), fill_ms.append(st["fill_ms"]), walls.append(w)
        count_ms, fill_ms, walls = count_ms[1:], fill_ms[1:], walls[1:]
        tbs = st["bytes"] / (np.median(fill_ms) * 1e-3) / 1e12
        print(f"  shared_factor={int(shared)}: {total:,} rows, {st['bytes'] / 1e9:.2f} GB written; ms, median (min - max) of {repeats}")
        print(f"    count + scan (HIP events) {mmm(count_ms)}   fill (HIP events) {mmm(fill_ms)}   whole call (wall) {mmm(walls)}")
        print(f"    fill: {tbs:.2f} TB/s = {100 * tbs / STORE_BOUND_TBS:.0f} % of the {STORE_BOUND_TBS} TB/s HBM store bound", flush=True)


def upload(table):
    return {k: torch.from_numpy(v).cuda() for k, v in table.items()}


def small(d, persons_n, repeats):
    regions, cats = d["regions"], d["categories"]
    _, _, min_person = sample.id_scheme(len(cats), d["place_count"])
    from_ms, hours, days = sample.year_interval(d["year"])
    host_persons = sc.persons(regions, persons_n, min_person)
    dev_persons = upload(host_persons)
    device = lambda: sample.generate_location_visits(dev_persons, regions, from_ms, hours, days)                     # noqa: E731
    host = lambda: upload(sc.location_visits(host_persons, regions, from_ms, hours, days))                           # noqa: E731
    got, want = device(), host()
    assert all(torch.equal(got[k], want[k]) for k in got), "device and restatement differ"
    rows = len(got["person_id"])
    del got, want
    t = {"device": [], "host": []}
    for _ in range(repeats):
        for name, fn in (("host", host), ("device", device)):
            w, out = wall(fn)
            del out
            t[name].append(w)
    print(f"{persons_n:,} persons, {rows:,} rows; wall ms, median (min - max) of {repeats} alternated runs")
    print(f"    numpy restatement + upload                 {mmm(t['host'])}")
    print(f"    device (count call + fill call)            {mmm(t['device'])}")
    print(f"    median host route / median device: {np.median(t['host']) / np.median(t['device']):.1f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--persons", type=int, default=None)
    ap.add_argument("--places", type=int, default=None)
    ap.add_argument("--small-persons", type=int, default=300_000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    d = sc.defaults()
    print(torch.cuda.get_device_name(0))
    shipped(d, a.persons or d["person_count"], a.places or d["place_count"], a.repeats)
    small(d, a.small_persons, a.repeats)


if __name__ == "__main__":
    main()
