#!/usr/bin/env python3
"""Times of the place deduplicator (csrc/dedup.hip) on a seeded case: by default 1 M places x 200 k confirmed places in
8 regions over city-sized areas (a 30 km square each); half the places are perturbed copies of a confirmed place of
their region, 0 - 120 m away with 0 - 8 edits of the name; radius 60 m and maxNameDifference 5, the parameters of
PlaceDeduplicatorTest.scala:35.  Device-memory inputs, one warm-up, then the banded kernel and the full-matrix A/B
partner (LOCREC_DEDUP_FULL_DP=1) ALTERNATED in one process, --repeats each: host-clock seconds of the whole call
(min / median / max and every repeat) and the HIP-event split grid / Levenshtein / compaction, candidates, same pairs.

The generator (perf_case) is what tests/test_gpu_dedup.py runs at a quarter of this size."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EARTH_RADIUS_METERS = 6371.0 * 1000.0
RADIUS_METERS, NAME_DIFFERENCE = 60.0, 5
# centres of the 8 regions: cities on both hemispheres, one next to the antimeridian
CENTRES = ((55.75, 37.62), (48.85, 2.35), (40.71, -74.0), (-33.87, 151.2), (35.68, 139.69), (-17.8, 179.95), (64.15, -21.94),
           (1.35, 103.82))
LETTERS = np.frombuffer("abcdefghijklmnopqrstuvwxyz абвгдежзиклмнопрстуя".encode("utf-16-le"), dtype=np.uint16)
MAX_NAME = 26


def offset_by(lat, lon, north_m, east_m):
    """Small offsets in metres on the sphere (city scale: the flat approximation is good to centimetres)."""
    lat2 = lat + np.degrees(north_m / EARTH_RADIUS_METERS)
    lon2 = lon + np.degrees(east_m / (EARTH_RADIUS_METERS * np.cos(np.radians(lat))))
    return np.clip(lat2, -90.0, 90.0), (lon2 + 180.0) % 360.0 - 180.0


def csr_of(chars, lengths):
    """chars[n, MAX_NAME + 1] with `lengths` valid units per row -> (offsets, units)"""
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    mask = np.arange(chars.shape[1])[None, :] < lengths[:, None]
    return off, np.ascontiguousarray(chars[mask], dtype=np.uint16)


def perf_case(n_places, n_confirmed, seed=0xDED0, regions=8, side_meters=30_000.0):
    """-> (places, confirmed): dicts of id, region_id, latitude, longitude, name_offsets, name_units (lower-case CSR)."""
    rng = np.random.default_rng(seed)
    c_region = rng.integers(0, regions, n_confirmed)
    centre = np.array(CENTRES[:regions])
    c_lat, c_lon = offset_by(centre[c_region, 0], centre[c_region, 1], rng.uniform(-0.5, 0.5, n_confirmed) * side_meters,
                             rng.uniform(-0.5, 0.5, n_confirmed) * side_meters)
    c_len = rng.integers(6, MAX_NAME - 1, n_confirmed)
    c_chars = LETTERS[rng.integers(0, len(LETTERS), (n_confirmed, MAX_NAME + 1))]
    # places: the even rows copy a confirmed place of (therefore) their own region, the odd rows are new
    src = rng.integers(0, n_confirmed, n_places)
    copy = (np.arange(n_places) % 2 == 0)
    p_region = np.where(copy, c_region[src], rng.integers(0, regions, n_places))
    dist, bearing = rng.uniform(0.0, 120.0, n_places), rng.uniform(0.0, 2 * np.pi, n_places)
    k_lat, k_lon = offset_by(c_lat[src], c_lon[src], dist * np.cos(bearing), dist * np.sin(bearing))
    n_lat, n_lon = offset_by(centre[p_region, 0], centre[p_region, 1], rng.uniform(-0.5, 0.5, n_places) * side_meters,
                             rng.uniform(-0.5, 0.5, n_places) * side_meters)
    p_lat, p_lon = np.where(copy, k_lat, n_lat), np.where(copy, k_lon, n_lon)
    p_chars = np.where(copy[:, None], c_chars[src], LETTERS[rng.integers(0, len(LETTERS), (n_places, MAX_NAME + 1))])
    p_len = np.where(copy, c_len[src], rng.integers(6, MAX_NAME - 1, n_places))
    edits = np.where(copy, rng.integers(0, 9, n_places), 0)       # 0 - 8: substitutions, the last one an edit of the length
    tail = (edits > 0) & (rng.random(n_places) < 0.5)
    for t in range(8):
        hit = np.flatnonzero(edits - tail > t)
        p_chars[hit, rng.integers(0, p_len[hit])] = ord("#") + t
    p_len = np.where(tail, p_len + np.where(rng.random(n_places) < 0.5, 1, -1), p_len)   # append a unit / drop the last
    p_off, p_units = csr_of(p_chars, p_len)
    c_off, c_units = csr_of(c_chars, c_len)
    places = dict(id=1_000_000_000 + np.arange(n_places, dtype=np.int64), region_id=p_region.astype(np.int64) * 10 - 3,
                  latitude=p_lat, longitude=p_lon, name_offsets=p_off, name_units=p_units)
    confirmed = dict(id=np.arange(n_confirmed, dtype=np.int64), region_id=c_region.astype(np.int64) * 10 - 3,
                     latitude=c_lat, longitude=c_lon, name_offsets=c_off, name_units=c_units)
    return places, confirmed


def mmm(xs):
    xs = np.asarray(xs, np.float64)
    return f"{xs.min():.4f} / {np.median(xs):.4f} / {xs.max():.4f}"


def main():
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    dd = pkg.deduplicator
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--places", type=int, default=1_000_000)
    ap.add_argument("--confirmed", type=int, default=200_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    t0 = time.perf_counter()
    places, confirmed = perf_case(args.places, args.confirmed)
    print(f"{torch.cuda.get_device_name(0)}; case built on the host in {time.perf_counter() - t0:.1f} s; "
          f"LOCREC_DEDUP_PAIR_BUDGET={os.environ.get('LOCREC_DEDUP_PAIR_BUDGET', 'default (2^26)')}")

    def dev(d):
        return {k: torch.as_tensor(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for k, v in d.items()}
    p, c = dev(places), dev(confirmed)

    def run(full_dp):
        if full_dp:
            os.environ["LOCREC_DEDUP_FULL_DP"] = "1"
        else:
            os.environ.pop("LOCREC_DEDUP_FULL_DP", None)
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = dd.find_duplicate_places(p, c, RADIUS_METERS, NAME_DIFFERENCE)
        torch.cuda.synchronize()
        return time.perf_counter() - t, out, dd.find_duplicate_places_stats()

    _, base, st = run(False)                                   # warm-up of both, and the two must agree
    _, other, _ = run(True)
    assert all(torch.equal(a, b) for a, b in zip(base, other)), "banded and full-matrix results differ"
    print(f"{args.places:,} places x {args.confirmed:,} confirmed places, 8 regions, radius {RADIUS_METERS:g} m, "
          f"maxNameDifference {NAME_DIFFERENCE}: {st['candidates']:,} candidates (within the radius, other id) in "
          f"{st['chunks']} chunk(s) -> {st['same']:,} same pairs; rows of dropDuplicates: {int(base[3].sum()):,}")
    secs, phases = {False: [], True: []}, {False: [], True: []}
    for _ in range(args.repeats):
        for full_dp in (False, True):                          # alternated
            t, _, s = run(full_dp)
            secs[full_dp].append(t)
            phases[full_dp].append((s["grid_ms"], s["lev_ms"], s["compact_ms"]))
    os.environ.pop("LOCREC_DEDUP_FULL_DP", None)
    for full_dp, name in ((False, "banded (default)"), (True, "full matrix (LOCREC_DEDUP_FULL_DP=1)")):
        ph = np.array(phases[full_dp])
        print(f"{name}: whole call, seconds min / median / max over {args.repeats}: {mmm(secs[full_dp])}")
        print(f"    every repeat, seconds      {' '.join(f'{t:.4f}' for t in secs[full_dp])}")
        for k, what in enumerate(("grid (region ranks, keys, sorts, both walks)", "Levenshtein over the candidates", "compaction")):
            print(f"    HIP-event ms, {what:<44} {mmm(ph[:, k])}")
    ratio = np.array(secs[False]) / np.array(secs[True])
    print(f"banded / full matrix, whole call, per repeat: {mmm(ratio)}  (the banded kernel stays the default if <= 1)")
    print(f"Levenshtein phase alone, banded / full matrix (medians): "
          f"{np.median(np.array(phases[False])[:, 1]) / np.median(np.array(phases[True])[:, 1]):.3f}")


if __name__ == "__main__":
    main()
