"""Inputs of the pool-visitors tests (locrec_knn_pool_visitors_*): one mixed batch of visitors over a pool of indexes.  Seeded,
no GPU.  The members are the smallest shapes at which the shared launches can go wrong - those of tests/test_gpu_knn_pool.py's
datasets(), rebuilt here, and a member without persons - and the visitors are interleaved in call order.  Every shape claim
is asserted in tests/test_knn_pool_visitor_cases.py."""
import functools

import numpy as np

import knn_visitor_cases as vc

PW, CW = 0.4, 0.6
KS = (2_000_000, 3_000, 50)      # every member shares; member 3 (4,200 persons) delegated; all delegated
FINISH_TILE, SEG_RATERS, QT, FILL_BLOCK, BATCH_MAX_K = 2048, 4096, 16, 256, 1024   # csrc/knn_large.hip, include/locrec.h
ASKED = {0: 2, 1: 2, 2: 37, 3: 2, 4: 1, 6: 1}    # visitors a member; member 5 is asked by nobody
LONG_ENTRIES = 300               # place entries, inside the dimensions, of member 2's long visitor


def with_ratings(d, seed=3, popular=None, none=False):
    """Every person rates the places of its place vector.  popular: EVERY person also rates that place; none: no rating
    rows at all."""
    rng = np.random.default_rng(seed)
    d = dict(d)
    n = len(d["person_ids"])
    if none:
        d["r_rowptr"], d["r_place"], d["r_rating"] = np.zeros(n + 1, np.int64), np.empty(0, np.int64), np.empty(0, np.int64)
        return d
    ptr, idx = d["p_rowptr"], d["p_idx"].astype(np.int64)
    if popular is not None:
        rows = [np.union1d(idx[ptr[i]:ptr[i + 1]], [popular]) for i in range(n)]
        ptr = np.zeros(n + 1, np.int64)
        np.cumsum([len(r) for r in rows], out=ptr[1:])
        idx = np.concatenate(rows)
    d["r_rowptr"], d["r_place"] = ptr.copy(), idx
    d["r_rating"] = rng.integers(1, 6, size=len(idx)).astype(np.int64)
    return d


def synth():
    import __graft_entry__ as g
    g.load_package()
    from locations_recommender_amd import synth as s
    return s


@functools.lru_cache(maxsize=None)
def members():
    """0: 200 persons (one scan block), integer counts   1: 257 persons (two blocks), fp64 values: the GENERIC format, no
    renumbering, another p_dim   2: 3,000 persons, p_dim 5,000, more than 2,048 rated places (two finish tiles)   3: 4,200
    persons who all rate place 7 (two segments of kSegRaters)   4: nobody rated anything   5: asked by nobody   6: 0 persons."""
    s = synth()
    empty = dict(person_ids=np.zeros(0, np.int64), p_rowptr=np.zeros(1, np.int64), p_idx=np.zeros(0, np.int32), p_val=np.zeros(0),
                 p_dim=300, c_rowptr=np.zeros(1, np.int64), c_idx=np.zeros(0, np.int32), c_val=np.zeros(0), c_dim=20)
    return (with_ratings(s.small_knn_dataset(n=200, p_dim=300, seed=21), 1),
            with_ratings(s.small_knn_dataset(n=257, p_dim=700, seed=22, integer=False), 2),
            with_ratings(s.small_knn_dataset(n=3000, p_dim=5000, seed=23), 3),
            with_ratings(s.small_knn_dataset(n=4200, p_dim=64, seed=24), 4, popular=7),
            with_ratings(s.small_knn_dataset(n=200, p_dim=300, seed=25), none=True),
            with_ratings(s.small_knn_dataset(n=200, p_dim=300, seed=26), 6),
            with_ratings(empty, none=True))


def rated_places(d):
    return len(np.unique(d["r_place"]))


def way(k, n):
    """knn_pool_visitors_way of csrc/knn_pool_visitors_plan.h."""
    if n <= 0:
        return "empty"
    return "shared" if k > BATCH_MAX_K and k >= n else "delegated"


def _pool_of_vectors(m, count, seed):
    """count rating vectors in member m's numbering that are no rows of it (another seed of the same generator)."""
    ds = members()
    src = synth().small_knn_dataset(n=count, p_dim=ds[m]["p_dim"], seed=seed, integer=m != 1)
    return [vc.row_of(src, r) for r in range(count)]


@functools.lru_cache(maxsize=None)
def visitors():
    """-> (index_of int32[nv], the visitors as dicts, names: position of the special ones).  37 visitors of member 2 (three
    waves, the last tile partial), 1 - 2 of members 0, 1, 3, 4 and 6, interleaved; every visitor has entries beyond its
    member's dimensions; `long`: a visitor of member 2 with more than 256 place entries inside the dimensions, in member 2's
    first tile (wave 0, whose other tiles are short); `all_beyond`: a visitor of member 0 whose place entries all lie beyond
    its dimensions; `shared`: ONE vector asked of members 0 and 1 (an entry at 450: inside member 1's 700 dimensions, beyond
    member 0's 300); `twice`: one vector asked twice of member 2."""
    ds = members()
    rng = np.random.default_rng(5)
    gi = np.concatenate([np.full(c, m, np.int32) for m, c in ASKED.items()])
    gi = gi[rng.permutation(len(gi))]
    c_dim = ds[0]["c_dim"]
    out, names = [None] * len(gi), {}
    # members 3, 4 and 6; the own visitor of member 1
    for m in (3, 4, 6):
        for j, (pos, v) in enumerate(zip(np.flatnonzero(gi == m), _pool_of_vectors(m, ASKED[m], 100 + m))):
            out[pos] = vc.with_beyond(v, ds[m]["p_dim"], c_dim, j + m)
    # ONE vector for members 0 and 1: integer counts (member 0 renumbers), indices below 300 and one at 450
    base = _pool_of_vectors(0, 1, 131)[0]
    shared = vc.with_beyond(dict(base, p_idx=np.r_[base["p_idx"], 450].astype(np.int32), p_val=np.r_[base["p_val"], 3.0]),
                            ds[1]["p_dim"], c_dim, 1)
    at0, at1 = np.flatnonzero(gi == 0), np.flatnonzero(gi == 1)
    out[at0[0]], out[at1[0]] = shared, shared
    names["shared"] = (int(at0[0]), int(at1[0]))
    out[at1[1]] = vc.with_beyond(_pool_of_vectors(1, 1, 132)[0], ds[1]["p_dim"], c_dim, 2)
    # all place entries beyond member 0's dimensions
    cat = _pool_of_vectors(0, 1, 133)[0]
    out[at0[1]] = dict(p_idx=np.array([300, 304, 1999], np.int32), p_val=np.array([2.0, 1.0, 5.0]),
                       c_idx=np.r_[cat["c_idx"], c_dim + 2].astype(np.int32), c_val=np.r_[cat["c_val"], 1.0])
    names["all_beyond"] = int(at0[1])
    # member 2: the long visitor first (its first tile), one vector twice (in different tiles), 34 others
    at2 = np.flatnonzero(gi == 2)
    vs = _pool_of_vectors(2, 35, 134)
    p_dim = ds[2]["p_dim"]
    long_idx = np.sort(np.random.default_rng(6).choice(p_dim, LONG_ENTRIES, replace=False)).astype(np.int32)
    long = dict(vs[0], p_idx=long_idx, p_val=(1.0 + np.arange(LONG_ENTRIES) % 7).astype(np.float64))
    mine = [long] + vs[1:35] + [vs[3]] + [vs[5]]
    mine = mine[:37]
    assert len(mine) == 37
    for j, (pos, v) in enumerate(zip(at2, mine)):
        out[pos] = vc.with_beyond(v, p_dim, c_dim, j)
    out[at2[35]] = out[at2[3]]        # the same vector, beyond entries included: tile 0 and tile 2
    names["long"] = int(at2[0])
    names["twice"] = (int(at2[3]), int(at2[35]))
    assert all(v is not None for v in out)
    return gi, out, names


def arrays(vs=None):
    """The six CSR arrays of the visitors (all of them by default)."""
    return vc.csr(visitors()[1] if vs is None else vs)


def of_member(m):
    """(positions in the call, ascending; the CSR arrays) of member m's visitors."""
    gi, vs, _ = visitors()
    at = np.flatnonzero(gi == m)
    return at, vc.csr([vs[i] for i in at])


def staged_lengths():
    """[2][nv]: the entries of each visitor inside its member's dimensions (what the stage keeps)."""
    gi, vs, _ = visitors()
    ds = members()
    return np.array([[int(np.sum(v["p_idx"] < ds[m]["p_dim"])) for m, v in zip(gi, vs)],
                     [int(np.sum(v["c_idx"] < ds[m]["c_dim"])) for m, v in zip(gi, vs)]])


def beyond_entries():
    gi, vs, _ = visitors()
    return sum(len(v["p_idx"]) + len(v["c_idx"]) for v in vs) - int(staged_lengths().sum())


def places_table():
    ids = np.arange(-5, max(d["p_dim"] for d in members()) + 5, dtype=np.int64)
    return ids, ids % 3


def targets(seed):
    """A target region per visitor; 99: a region no place belongs to."""
    gi, _, names = visitors()
    t = np.random.default_rng(seed).choice([0, 1, 2, 99], len(gi)).astype(np.int64)
    t[names["twice"][0]], t[names["twice"][1]] = 0, 1      # the vector asked twice, two targets
    t[0] = 99
    return t


def exclusion_lists():
    """(offsets[nv + 1], place ids): every visitor's rated places (its place indices), every third visitor's list empty."""
    gi, vs, _ = visitors()
    lists = [v["p_idx"].astype(np.int64) if i % 3 else np.zeros(0, np.int64) for i, v in enumerate(vs)]
    off = np.zeros(len(vs) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    return off, np.concatenate(lists)
