"""Inputs and expected values of the visitors' tests (locrec_knn_visitors_*): rating vectors that are no rows of the index.
Seeded, no GPU.  A visitor is a dict p_idx / p_val / c_idx / c_val in the index's ORIGINAL numbering; the expected value of
every call is the oracle's answer for the visitor on the data set with the visitor appended under an id no person has
(index_plus_visitor).  The oracle takes indices beyond p_dim / c_dim as they are: they enter the vector length only."""
import functools

import numpy as np

VISITOR_ID = 999_999
N_ALL, P_DIM, SEED, N_VISITORS = 3000, 600, 11, 40
KS = (1, 50, 1024, 1025, N_ALL - N_VISITORS - 1, N_ALL - N_VISITORS, 2_000_000)


def row_of(d, r):
    pa, pb = d["p_rowptr"][r], d["p_rowptr"][r + 1]
    ca, cb = d["c_rowptr"][r], d["c_rowptr"][r + 1]
    return dict(p_idx=d["p_idx"][pa:pb].copy(), p_val=d["p_val"][pa:pb].copy(),
                c_idx=d["c_idx"][ca:cb].copy(), c_val=d["c_val"][ca:cb].copy())


def from_rows(d, rows, ids=None):
    """The data set of the listed rows of d (vectors only)."""
    vs = [row_of(d, r) for r in rows]
    out = csr(vs)
    return dict(person_ids=np.asarray(d["person_ids"])[rows].astype(np.int64) if ids is None else np.asarray(ids, np.int64),
                p_rowptr=out[0], p_idx=out[1], p_val=out[2], p_dim=d["p_dim"],
                c_rowptr=out[3], c_idx=out[4], c_val=out[5], c_dim=d["c_dim"])


def csr(visitors):
    """(p_rowptr, p_idx, p_val, c_rowptr, c_idx, c_val) of a list of visitors."""
    def fam(k):
        ptr = np.zeros(len(visitors) + 1, np.int64)
        np.cumsum([len(v[k + "_idx"]) for v in visitors], out=ptr[1:])
        idx = np.concatenate([v[k + "_idx"] for v in visitors]).astype(np.int32) if visitors else np.zeros(0, np.int32)
        val = np.concatenate([v[k + "_val"] for v in visitors]).astype(np.float64) if visitors else np.zeros(0, np.float64)
        return ptr, idx, val
    return fam("p") + fam("c")


def index_plus_visitor(d, v):
    """d with the visitor appended as the person VISITOR_ID (the dimensions stay d's: the oracle does not read them)."""
    assert VISITOR_ID not in set(np.asarray(d["person_ids"]).tolist())
    out = dict(d)
    out["person_ids"] = np.r_[np.asarray(d["person_ids"], np.int64), VISITOR_ID]
    for k in ("p", "c"):
        out[k + "_rowptr"] = np.r_[d[k + "_rowptr"], d[k + "_rowptr"][-1] + len(v[k + "_idx"])].astype(np.int64)
        out[k + "_idx"] = np.r_[d[k + "_idx"], v[k + "_idx"]].astype(np.int32)
        out[k + "_val"] = np.r_[d[k + "_val"], v[k + "_val"]].astype(np.float64)
    for k in ("r_rowptr", "r_place", "r_rating"):
        out.pop(k, None)
    if "r_rowptr" in d:  # the visitor has no rating rows
        out["r_rowptr"] = np.r_[d["r_rowptr"], d["r_rowptr"][-1]].astype(np.int64)
        out["r_place"], out["r_rating"] = d["r_place"], d["r_rating"]
    return out


def with_beyond(v, p_dim, c_dim, j):
    """v with two place entries and one category entry beyond the dimensions (integer counts)."""
    return dict(p_idx=np.r_[v["p_idx"], p_dim + 3 + j, p_dim + 1000 + 7 * j].astype(np.int32),
                p_val=np.r_[v["p_val"], 2.0 + j % 5, 1.0 + j % 3],
                c_idx=np.r_[v["c_idx"], c_dim + j].astype(np.int32), c_val=np.r_[v["c_val"], 3.0 + j % 4])


def without_beyond(v, p_dim, c_dim):
    kp, kc = v["p_idx"] < p_dim, v["c_idx"] < c_dim
    return dict(p_idx=v["p_idx"][kp], p_val=v["p_val"][kp], c_idx=v["c_idx"][kc], c_val=v["c_val"][kc])


def explicit_ratings(d):
    """d with its place vectors as explicit placeRatings rows (so that a visitor can be appended without any)."""
    return dict(d, r_rowptr=np.asarray(d["p_rowptr"], np.int64), r_place=np.asarray(d["p_idx"], np.int64),
                r_rating=np.asarray(d["p_val"], np.int64))


@functools.lru_cache(maxsize=None)
def base(integer=True):
    """(index data of 2,960 persons with explicit ratings, the 40 visitors taken out of the 3,000): every visitor holds
    two place entries and one category entry beyond the dimensions."""
    import __graft_entry__ as g
    g.load_package()
    from locations_recommender_amd import synth
    full = synth.small_knn_dataset(n=N_ALL, p_dim=P_DIM, seed=SEED, integer=integer)
    out = np.arange(N_ALL - N_VISITORS, N_ALL)           # the last 40 rows: each has more than 1,025 candidates
    keep = np.setdiff1d(np.arange(N_ALL), out)
    d = from_rows(full, keep)
    if integer:
        d = explicit_ratings(d)
    else:  # (ratings are integer counts whatever the vectors hold)
        d = dict(d, r_rowptr=np.asarray(d["p_rowptr"], np.int64), r_place=np.asarray(d["p_idx"], np.int64),
                 r_rating=np.floor(d["p_val"]).astype(np.int64))
    visitors = [with_beyond(row_of(full, r), P_DIM, full["c_dim"], j) for j, r in enumerate(out)]
    return d, visitors


def all_categories_visitor(d):
    """Holds every category: every person (all have a category vector of positive counts) is a candidate."""
    return dict(p_idx=np.array([0], np.int32), p_val=np.array([1.0]),
                c_idx=np.arange(d["c_dim"], dtype=np.int32), c_val=np.ones(d["c_dim"]))


def nobody_visitor(d):
    """Indices nobody holds: beyond the dimensions in both families."""
    return dict(p_idx=np.array([d["p_dim"] + 5], np.int32), p_val=np.array([2.0]),
                c_idx=np.array([d["c_dim"] + 1], np.int32), c_val=np.array([1.0]))


@functools.lru_cache(maxsize=None)
def expected_similar(integer, j, k, pw=0.5, cw=0.5):
    import oracle_binding as ob
    d, visitors = base(integer)
    return ob.knn_similar(index_plus_visitor(d, visitors[j]), VISITOR_ID, pw, cw, k)


@functools.lru_cache(maxsize=None)
def expected_recommend(integer, j, k, pw=0.5, cw=0.5):
    import oracle_binding as ob
    d, visitors = base(integer)
    return ob.knn_recommend(index_plus_visitor(d, visitors[j]), VISITOR_ID, pw, cw, k)


def oracle_similar(d, v, pw, cw, k):
    import oracle_binding as ob
    return ob.knn_similar(index_plus_visitor(d, v), VISITOR_ID, pw, cw, k)


def oracle_recommend(d, v, pw, cw, k):
    import oracle_binding as ob
    return ob.knn_recommend(index_plus_visitor(d, v), VISITOR_ID, pw, cw, k)
