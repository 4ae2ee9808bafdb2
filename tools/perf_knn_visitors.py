#!/usr/bin/env python3
"""KNN for visitors (locrec_knn_visitors_recommend_batch) against the parent's way to serve the same vectors, on bench.py's
KNN input at configs[1] (1 M persons x 100 k places, seed 0x5EED0002; placeRatings from the place index, rating
1 + place % 5):

  visitors   1,024 rows drawn with a fixed seed are taken OUT of the data set; the index holds the others, the rows are
             asked as visitors (host arrays)
  persons    the index over ALL rows (the "plus-visitors" index, without the rebuild the parent would need per
             visitor), the same rows asked through locrec_knn_recommend_batch by their ids

16 and 1,024 of them at K = 50 and K = 2,000,000.  Both forms are warmed first, then alternated --repeats times with a
synchronise around every timed call; ms per call as min / median / max.  Output arrays are kept from call to call.
With the handles' kernel profile on, the K = 2,000,000 runs also give the scan kernel's own time per tile of 16:
lkv_scan of the visitors against lkb_scan of the persons (at K = 50 the persons take the head / tail scan: no partner)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
from locations_recommender_amd import _lib as L, synth  # noqa: E402
import knn_visitor_cases as vc  # noqa: E402

PW = CW = 0.5


def with_ratings(d):
    d = dict(d)
    d["r_rowptr"] = d["p_rowptr"]
    d["r_place"] = d["p_idx"].astype(np.int64)
    d["r_rating"] = 1 + d["r_place"] % 5
    return d


def make_index(d):
    return pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"], d["c_rowptr"], d["c_idx"],
                        d["c_val"], d["c_dim"], d["r_rowptr"], d["r_place"], d["r_rating"])


def without_rows(d, out):
    """d without the listed rows (vectors only)"""
    keep = np.ones(len(d["person_ids"]), bool)
    keep[out] = False
    res = dict(person_ids=d["person_ids"][keep], p_dim=d["p_dim"], c_dim=d["c_dim"])
    for f in ("p", "c"):
        lens = np.diff(d[f + "_rowptr"])
        ek = np.repeat(keep, lens)
        res[f + "_idx"], res[f + "_val"] = d[f + "_idx"][ek], d[f + "_val"][ek]
        res[f + "_rowptr"] = np.r_[0, np.cumsum(lens[keep])].astype(np.int64)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--persons", type=int, default=1_000_000)
    ap.add_argument("--places", type=int, default=100_000)
    args = ap.parse_args()
    n = args.persons
    full = synth.knn_dataset(n, args.places, 0x5EED0002)
    out = np.sort(np.random.default_rng(1024).choice(n, 1024, replace=False))
    visitors = [vc.row_of(full, r) for r in out]
    ix_v = make_index(with_ratings(without_rows(full, out)))
    ix_p = make_index(with_ratings(full))
    lib = L.lib()
    buf = [np.empty(1 << 20, np.int64), np.empty(1 << 20, np.float64)]

    def call(fn, nq):
        off = np.zeros(nq + 1, np.int64)
        while True:
            cap = C.c_int64(len(buf[0]))
            L.check(fn(off, cap))
            if cap.value <= len(buf[0]):
                return off, buf[0][:off[-1]], buf[1][:off[-1]]
            buf[:] = [np.empty(cap.value, np.int64), np.empty(cap.value, np.float64)]

    recs = []
    for nv in (16, 1024):
        arrays = vc.csr(visitors[:nv])
        nvv, ptrs, mem, keep = pkg.KnnIndex._visitor_args(*arrays)
        pids = np.ascontiguousarray(full["person_ids"][out[:nv]], np.int64)
        for k in (50, 2_000_000):
            bad = C.c_int64(-1)

            def as_visitors():
                return call(lambda off, cap: lib.locrec_knn_visitors_recommend_batch(
                    ix_v._h, nv, *ptrs, mem, PW, CW, k, L.ptr(off, C.c_int64), L.ptr(buf[0], C.c_int64), L.ptr(buf[1], C.c_double),
                    C.byref(cap), C.byref(bad)), nv)

            def as_persons():
                return call(lambda off, cap: lib.locrec_knn_recommend_batch(
                    ix_p._h, nv, L.ptr(pids, C.c_int64), PW, CW, k, L.ptr(off, C.c_int64), L.ptr(buf[0], C.c_int64),
                    L.ptr(buf[1], C.c_double), C.byref(cap)), nv)

            for _ in range(2):  # warm both (workspaces grown, output arrays sized)
                v = [a.copy() for a in as_visitors()]
                p = [a.copy() for a in as_persons()]
            # the other visitors are persons of the plus-visitors index: the two answers differ, their sizes hardly
            tv, tp, sv, sp = [], [], [], []
            for ix in (ix_v, ix_p):
                ix.profile_enable(True)
                ix.profile_read()
            for _ in range(args.repeats):
                for ix, fn, ts, scan in ((ix_v, as_visitors, tv, sv), (ix_p, as_persons, tp, sp)):
                    ix.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ix.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                    ms, launches = ix.profile_read()
                    scan.append(ms / max(1, launches))
            for ix in (ix_v, ix_p):
                ix.profile_enable(False)
            st = pkg.KnnIndex.visitors_stats()
            f3 = lambda a: f"{min(a):.3f} / {float(np.median(a)):.3f} / {max(a):.3f}"
            line = (f"{nv} vectors K={k:,}: visitors {f3(tv)} ms, persons of the plus-visitors index {f3(tp)} ms "
                    f"(min / median / max over {args.repeats}); rows {len(v[1]):,} vs {len(p[1]):,}; "
                    f"visitor tiles {st['tiles']} ({st['tiles_all']} without a top-K)")
            if k >= n:
                line += f"; scan kernel per tile: lkv_scan {f3(sv)} ms, lkb_scan {f3(sp)} ms"
            print(line, flush=True)
            recs.append({"vectors": nv, "k": k, "visitors_ms": sorted(round(x, 3) for x in tv),
                         "persons_ms": sorted(round(x, 3) for x in tp),
                         "lkv_scan_ms_per_tile": sorted(round(x, 4) for x in sv) if k >= n else None,
                         "lkb_scan_ms_per_tile": sorted(round(x, 4) for x in sp) if k >= n else None})
    ix_v.close()
    ix_p.close()
    print(json.dumps({"metric": "knn_visitors", "persons": n, "places": args.places, "results": recs}), flush=True)


if __name__ == "__main__":
    main()
