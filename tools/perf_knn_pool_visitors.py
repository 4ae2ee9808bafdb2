#!/usr/bin/env python3
"""One pool call for visitors (locrec_knn_pool_visitors_recommend_ranked_batch) against one
locrec_knn_visitors_recommend_ranked_batch call per distinct member in sequence - how a queue of cold-start persons over many
region-set indexes was served before the pool form - for the same vectors in the same process, at the shipped
K = 2,000,000 (both warmed first, alternated, repeated; min / median / max of wall clock, the device synchronised around
every call):

  workloads   tools/perf_knn_pool.py's: 12 and 64 members of ~3,000 persons (synth.knn_dataset(3000, 300)) and 8 members of
              ~200,000 persons (synth.knn_dataset(200000, 10000)), with 1, 4 and 16 visitors per member; a visitor is a
              row of another data set of the member's shape (another seed), every person rating the places of its vector

The rows go to --out (default profiles/knn_pool_visitors_perf.txt) and to the standard output.  --small-only / --large-only
run one of the two sizes."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
from locations_recommender_amd import synth  # noqa: E402

PW, CW, K, TOP = 0.5, 0.5, 2_000_000, 10
WORKLOADS = (("12 members of ~3 k persons", 3_000, 300, 12), ("64 members of ~3 k persons", 3_000, 300, 64),
             ("8 members of ~200 k persons", 200_000, 10_000, 8))


def member(persons, places, seed):
    d = synth.knn_dataset(persons, places, seed)
    rating = np.random.default_rng(seed).integers(1, 6, size=len(d["p_idx"])).astype(np.int64)
    return d, pkg.KnnIndex(d["person_ids"], d["p_rowptr"], d["p_idx"], d["p_val"], d["p_dim"], d["c_rowptr"], d["c_idx"],
                           d["c_val"], d["c_dim"], d["p_rowptr"].copy(), d["p_idx"].astype(np.int64), rating)


def visitors_of(places, seed, count):
    """count rating vectors in a member's numbering that are no rows of it: (six CSR arrays)"""
    src = synth.knn_dataset(2_000, places, seed)
    p, c = src["p_rowptr"], src["c_rowptr"]
    return (p[:count + 1].copy(), src["p_idx"][:p[count]].copy(), src["p_val"][:p[count]].copy(),
            c[:count + 1].copy(), src["c_idx"][:c[count]].copy(), src["c_val"][:c[count]].copy())


def concat(csrs):
    """ONE CSR over the visitors of all members, member after member"""
    out = []
    for f in (0, 3):
        ptr, base = [np.zeros(1, np.int64)], 0
        for c in csrs:
            ptr.append(c[f][1:] + base)
            base += c[f][-1]
        out += [np.concatenate(ptr), np.concatenate([c[f + 1] for c in csrs]), np.concatenate([c[f + 2] for c in csrs])]
    return out


def head(csr, count):
    p, c = csr[0], csr[3]
    return (p[:count + 1], csr[1][:p[count]], csr[2][:p[count]], c[:count + 1], csr[4][:c[count]], csr[5][:c[count]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_pool_visitors_perf.txt"))
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--large-only", action="store_true")
    args = ap.parse_args()
    import torch
    lines = ["# tools/perf_knn_pool_visitors.py: per-member = one locrec_knn_visitors_recommend_ranked_batch call per distinct member "
             "in sequence, pool = one locrec_knn_pool_visitors_recommend_ranked_batch call;",
             f"# K = {K}, top {TOP}; min / median / max of wall clock in ms over {args.repeats} alternated repeats, the device "
             "synchronised around every call; ratio = per-member median / pool median (above 1: the pool is faster)"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for name, persons, places, n in WORKLOADS:
        if (args.small_only and persons > 10_000) or (args.large_only and persons <= 10_000):
            continue
        made = [member(persons, places, 0x900 + i) for i in range(n)]
        ixs = [m[1] for m in made]
        pool = pkg.KnnPool(ixs)
        place_ids = np.arange(40, 40 + places, dtype=np.int64)
        regions = place_ids % 3
        rng = np.random.default_rng(64)
        drawn = [visitors_of(places, 0xA00 + i, 16) for i in range(n)]
        for per_member in (1, 4, 16):
            gi = np.repeat(np.arange(n, dtype=np.int32), per_member)
            mine = [head(c, per_member) for c in drawn]
            everybody = concat(mine)
            tgt = rng.integers(0, 3, len(gi)).astype(np.int64)

            def timed(f):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = f()
                torch.cuda.synchronize()
                return time.perf_counter() - t0, r

            def per_member_calls():
                return timed(lambda: [ix.visitors_recommend_ranked_batch(*v, PW, CW, K, place_ids, regions,
                                                                         tgt[m * per_member:(m + 1) * per_member], TOP)
                                      for m, (ix, v) in enumerate(zip(ixs, mine))])

            def pool_call():
                return timed(lambda: pool.visitors_recommend_ranked_batch(gi, *everybody, PW, CW, K, place_ids, regions, tgt, TOP))

            for _ in range(2):  # warm both (workspaces, stages, row buffers)
                _, rb = per_member_calls()
                _, rp = pool_call()
            assert np.array_equal(np.concatenate([r[0] for r in rb]), rp[0])
            assert np.concatenate([r[1] for r in rb]).tobytes() == rp[1].tobytes()
            assert np.array_equal(np.concatenate([r[2] for r in rb]), rp[2]) and rp[2].max() > 0
            tb, tp = [], []
            for _ in range(args.repeats):
                tb.append(per_member_calls()[0])
                tp.append(pool_call()[0])
            st = pool.visitors_stats()
            tb, tp = np.asarray(tb) * 1e3, np.asarray(tp) * 1e3
            emit(f"{name}, {per_member:2d} visitors per member: per-member {tb.min():8.3f} / {np.median(tb):8.3f} / {tb.max():8.3f}, "
                 f"pool {tp.min():8.3f} / {np.median(tp):8.3f} / {tp.max():8.3f}, ratio {np.median(tb) / np.median(tp):5.2f}  "
                 f"[pool: {st['waves']} waves, {st['member_tiles']} member tiles, "
                 f"{st['stage_launches'] + st['fill_launches'] + st['scan_launches'] + st['aggregate_launches'] + st['finish_launches']} "
                 f"launches, {st['host_syncs']} waits, {st['readback_bytes']} bytes back]")
        pool.close()
        for ix in ixs:
            ix.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    append = args.large_only and os.path.exists(args.out)  # (the two sizes measured in two runs: one table)
    with open(args.out, "a" if append else "w") as f:
        f.write("\n".join(lines[2:] if append else lines) + "\n")


if __name__ == "__main__":
    main()
