#!/usr/bin/env python3
"""One pool call for SG visitors (locrec_sg_pool_visitors_recommend_ranked_batch) against one
locrec_sg_visitors_recommend_ranked_batch call per member in a loop - how a queue of cold-start persons over many region-set
graphs was served before the pool form - for the same visitors in the same process, at the shipped epsilon = 0.01 and 20
iterations (both warmed first, alternated, repeated; min / median / max of wall clock, the device synchronised around
every call):

  workloads   12 and 64 members of ~3,000 persons (synth.sg_dataset(3000, 300, 20)) and 8 members of ~200,000 persons
              (synth.sg_dataset(200000, 10000, 20)), 16 visitors per member; a visitor is a person of another data set of
              the member's shape (another seed) with the edges whose targets are live in the member

Both paths' outputs are compared for bit equality in the same run (their SHA-256 is printed; --dump DIR keeps both as
.npz).  The rows go to --out (default profiles/sg_pool_visitors_perf.txt) and to the standard output.  --small-only /
--large-only run one of the two sizes; --time-limit SECONDS ends the run (default 900)."""
import argparse
import hashlib
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
from locations_recommender_amd import synth  # noqa: E402

ALPHA, EPS, MAX_IT, TOP, PER_MEMBER = 0.15, 0.01, 20, 10, 16
WORKLOADS = (("12 members of ~3 k persons", 3_000, 300, 12), ("64 members of ~3 k persons", 3_000, 300, 64),
             ("8 members of ~200 k persons", 200_000, 10_000, 8))


def visitors_of(persons, places, seed, live, count):
    """count persons of another data set of the same shape as (edge_offsets, target_ids, weights): the edges whose targets
    are live in the member"""
    g = synth.sg_dataset(n_persons=min(persons, 2_000), n_places=places, n_categories=20, seed=seed)
    src, dst, w = g["source_id"], g["target_id"], g["balanced_weight"]
    first = int(g["first_person"])
    off, t, x = [0], [], []
    for p in range(first, first + count):
        own = (src == p) & np.isin(dst, live)
        assert own.any()
        t.append(dst[own])
        x.append(w[own])
        off.append(off[-1] + int(own.sum()))
    return np.array(off, np.int64), np.concatenate(t), np.concatenate(x)


def digest(rows):
    h = hashlib.sha256()
    for a in rows:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sg_pool_visitors_perf.txt"))
    ap.add_argument("--dump")
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--large-only", action="store_true")
    ap.add_argument("--time-limit", type=int, default=900)
    args = ap.parse_args()
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("perf_sg_pool_visitors.py: the time limit ran out"))
    signal.alarm(args.time_limit)
    import torch
    lines = ["# tools/perf_sg_pool_visitors.py: per-member = one locrec_sg_visitors_recommend_ranked_batch call per member in a loop, "
             "pool = one locrec_sg_pool_visitors_recommend_ranked_batch call;",
             f"# epsilon {EPS}, max {MAX_IT} iterations, top {TOP}, {PER_MEMBER} visitors per member; min / median / max of wall clock "
             f"in ms over {args.repeats} alternated repeats, the device synchronised around every call; ratio = per-member median / "
             "pool median (above 1: the pool is faster)"]

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    for name, persons, places, n in WORKLOADS:
        if (args.small_only and persons > 10_000) or (args.large_only and persons <= 10_000):
            continue
        sgs, mine = [], []
        for i in range(n):
            g = synth.sg_dataset(n_persons=persons, n_places=places, n_categories=20, seed=0x700 + i)
            sgs.append(pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"]))
            mine.append(visitors_of(persons, places, 0xB00 + i, np.unique(g["target_id"]), PER_MEMBER))
        pool = pkg.SgPool(sgs)
        place_ids = np.arange(40, 40 + places, dtype=np.int64)
        regions = place_ids % 3
        gi = np.repeat(np.arange(n, dtype=np.int32), PER_MEMBER)
        tgt = np.random.default_rng(64).integers(0, 3, len(gi)).astype(np.int64)
        off = np.r_[0, np.cumsum(np.concatenate([np.diff(m[0]) for m in mine]))].astype(np.int64)
        t, w = np.concatenate([m[1] for m in mine]), np.concatenate([m[2] for m in mine])

        def timed(f):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = f()
            torch.cuda.synchronize()
            return time.perf_counter() - t0, r

        def per_member_calls():
            return timed(lambda: [sg.visitors_recommend_ranked_batch(*m, ALPHA, EPS, MAX_IT, place_ids, regions,
                                                                     tgt[k * PER_MEMBER:(k + 1) * PER_MEMBER], TOP)
                                  for k, (sg, m) in enumerate(zip(sgs, mine))])

        def pool_call():
            return timed(lambda: pool.visitors_recommend_ranked_batch(gi, off, t, w, ALPHA, EPS, MAX_IT, place_ids, regions, tgt, TOP))

        for _ in range(3):  # warm both (batch buffers, stages, emit-row images)
            _, rb = per_member_calls()
            _, rp = pool_call()
        cnt = np.concatenate([r[2] for r in rb])
        keep = np.arange(TOP)[None, :] < cnt[:, None]
        wide = lambda a, fill: np.concatenate([np.pad(x, ((0, 0), (0, TOP - x.shape[1])), constant_values=fill) for x in a])
        loop_rows = (wide([r[0] for r in rb], -1)[keep], wide([r[1] for r in rb], 0.0)[keep], cnt, np.concatenate([r[3] for r in rb]),
                     np.concatenate([r[4] for r in rb]))
        pool_rows = (np.pad(rp[0], ((0, 0), (0, TOP - rp[0].shape[1])), constant_values=-1)[keep],
                     np.pad(rp[1], ((0, 0), (0, TOP - rp[1].shape[1])))[keep], rp[2], rp[3], rp[4])
        same = all(a.tobytes() == b.tobytes() for a, b in zip(loop_rows, pool_rows)) and cnt.max() > 0
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            tag = name.replace(" ", "_").replace("~", "")
            np.savez(os.path.join(args.dump, tag + "_loop.npz"), *loop_rows)
            np.savez(os.path.join(args.dump, tag + "_pool.npz"), *pool_rows)
        tb, tp = [], []
        for _ in range(args.repeats):
            tb.append(per_member_calls()[0])
            tp.append(pool_call()[0])
        st = pool.visitors_stats()
        tb, tp = np.asarray(tb) * 1e3, np.asarray(tp) * 1e3
        emit(f"{name}, {PER_MEMBER} visitors per member: per-member {tb.min():8.3f} / {np.median(tb):8.3f} / {tb.max():8.3f}, "
             f"pool {tp.min():8.3f} / {np.median(tp):8.3f} / {tp.max():8.3f}, ratio {np.median(tb) / np.median(tp):5.2f}  "
             f"[pool: {st['tile_waves']} waves, {st['member_tiles']} member tiles, {st['rounds']} rounds, {st['sweep_launches']} sweep + "
             f"{st['finalize_launches']} finalize + {st['begin_launches'] + st['set_up_launches']} set-up launches, {st['polls']} polls; "
             f"outputs {'equal bit for bit' if same else 'DIFFER'}: loop {digest(loop_rows)}, pool {digest(pool_rows)}]")
        assert same, "the pool call and the per-member calls differ"
        pool.close()
        for sg in sgs:
            sg.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    append = args.large_only and os.path.exists(args.out)  # (the two sizes measured in two runs: one table)
    with open(args.out, "a" if append else "w") as f:
        f.write("\n".join(lines[2:] if append else lines) + "\n")


if __name__ == "__main__":
    main()
