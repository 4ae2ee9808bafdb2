"""GPU: the ranked SG batch (csrc/sg_ranked.h, and the tile loop of csrc/sg_batch.hip that it drives) on the limits of its
tiles, its bitmap words, the ranker's paths behind it and its ids ("Limits of the rankers"; the inputs:
rank_limit_cases.py, checked on the CPU by test_rank_limit_cases.py).

The expected value is recommend_batch's host rows through mains.rank_recommendations_batch, as in test_gpu_sg_ranked.py:
ids, counts, probability bits, iterations and verdicts are equal.  In every test the first and the last request are
also checked end to end against the oracle (oracle.sg_recommend, then oracle.rank_recommendations): ids and counts
equal, probabilities within the suite's bar.  The limits (16, 64, 256, 65535) are literals."""
import ctypes as C

import numpy as np
import pytest

import rank_batch_cases as rb
import rank_limit_cases as rl
from test_gpu_sg_batch import ALPHA, RTOL
from test_gpu_sg_ranked import PLACE0, expected, pkg_stats, places_table, region_popcounts, same_all

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mains(pkg):
    from locations_recommender_amd import mains
    return mains


def ranked(mains, batch, place_ids, regions, targets, limit):
    """`expected` of test_gpu_sg_ranked.py from a recommend_batch that was run once for several limits."""
    off, ids, probs, its, conv = batch
    return mains.rank_recommendations_batch(off, ids, probs, place_ids, regions, targets, limit), its, conv, np.diff(off)


def check_ends_against_oracle(oracle, src, dst, w, v, t, eps, max_it, place_ids, regions, limit, got):
    """The first and the last request from the edges to the ranked rows by the oracle alone."""
    for i in (0, len(v) - 1):
        oi, op, oit, oconv = oracle.sg_recommend(src, dst, w, int(v[i]), ALPHA, eps, max_it)
        ri, rs = oracle.rank_recommendations(oi, op, place_ids, regions, int(t[i]), min(limit, len(oi)))
        n = int(got[2][i])
        assert n == len(ri) and np.array_equal(got[0][i, :n], ri), (i, int(v[i]), int(t[i]))
        np.testing.assert_allclose(got[1][i, :n], rs, rtol=RTOL, atol=0)
        assert (int(got[3][i]), bool(got[4][i])) == (oit, oconv)


def row_counts_by_the_c_entry(sg, v, eps, max_it, place_ids, regions, t, stride=3):
    from locations_recommender_amd import _lib as L
    n = len(v)
    oi, op = np.full((n, stride), -5, np.int64), np.full((n, stride), -5.0)
    cnt, rows = np.full(n, -5, np.int64), np.full(n, -5, np.int64)
    L.check(L.lib().locrec_sg_recommend_ranked_batch(
        sg._h, n, L.ptr(v, C.c_int64), ALPHA, eps, max_it, len(place_ids), L.ptr(place_ids, C.c_int64),
        L.ptr(regions, C.c_int64), L.ptr(t, C.c_int64), stride, L.ptr(oi, C.c_int64), L.ptr(op, C.c_double),
        L.ptr(cnt, C.c_int64), L.ptr(rows, C.c_int64), None, None))
    return rows


# ---- tiles narrower than 16 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,width", rl.NARROW_T, ids=[str(t) for t, _ in rl.NARROW_T])
def test_narrow_tiles(pkg, oracle, mains, monkeypatch, T, width):
    """uint16 columns address rows up to 65535, so a tile has min(16, 65535 - T) targets: 2 at T = 65533, 1 at 65534; at
    65535 the columns are int32 and a tile has 16 again.  The 17 distinct targets make 9, 17 and 2 tiles: a request's
    column is its distinct target's number modulo the WIDTH, a tile's target rows and row counters are the first `nb`
    of 16, and the tile's requests are those of `nb` distinct targets.
    Bites (tried): `u % tile_max` read as `u % 16` reads columns that no sweep of the tile advanced - T = 65533 and 65534
    fail at (0.01, 20), T = 65535 passes."""
    assert width == {65533: 2, 65534: 1, 65535: 16}[T]
    g = rl.sg_narrow_tile_graph(T)
    src, dst, w, v, t, pl, reg = (g[k] for k in ("src", "dst", "w", "targets", "target_regions", "place_ids", "regions"))
    on = pkg.SgGraph(src, dst, w)
    monkeypatch.setenv("LOCREC_SG_NO_COL16", "1")
    off = pkg.SgGraph(src, dst, w)
    monkeypatch.delenv("LOCREC_SG_NO_COL16")
    assert on.live_count() == T
    distinct = len(np.unique(v))
    assert distinct == 17
    for eps, max_it in ((0.01, 20), (0.01, 0)):
        batch = on.recommend_batch(v, ALPHA, eps, max_it)
        for limit in (10, 2 ** 40):
            want = ranked(mains, batch, pl, reg, t, limit)
            got = on.recommend_ranked_batch(v, ALPHA, eps, max_it, pl, reg, t, limit)
            st = pkg_stats(on)
            assert same_all(got, want), (eps, max_it, limit)
            assert st["tiles"] == -(-distinct // width)
            assert got[2][t == rl.NO_REGION].tolist() == [0] and got[2][t != rl.NO_REGION].min() > 0, got[2]
            if limit == 2 ** 40:
                assert st["emitted_rows"] == got[2].sum() > 0
            other = off.recommend_ranked_batch(v, ALPHA, eps, max_it, pl, reg, t, limit)
            assert pkg_stats(off)["tiles"] == 2
            assert rb.same(other[:3], got[:3]) and np.array_equal(other[3], got[3]) and np.array_equal(other[4], got[4])
        assert np.array_equal(row_counts_by_the_c_entry(on, v, eps, max_it, pl, reg, t), np.diff(batch[0]))
        check_ends_against_oracle(oracle, src, dst, w, v, t, eps, max_it, pl, reg, 10, on.recommend_ranked_batch(
            v, ALPHA, eps, max_it, pl, reg, t, 10))
    on.close()
    off.close()


# ---- single bits of the membership bitmap -------------------------------------------------------------------------------

@pytest.mark.parametrize("n_live,n_vertices", rl.BIT_SIZES)
def test_single_bits(pkg, oracle, mains, monkeypatch, n_live, n_vertices):
    """Every vertex is a region of its own with one table row, and a person and a place ask for every region: each bit
    of the bitmaps is a request's only member, on every emit row from 0 to m - 1, with m = n_vertices (no sweep: the
    source-only vertices are numbered behind the live ones and every vertex stands at 1 / V) and m = n_live (three
    sweeps) at 63, 64, 65, 255, 256 and 257.
    Bites (tried): `e0 < ne` read as `e0 + 63 < ne` in sg_rk_emit, which skips the last, partly filled word of the
    bitmap - every size fails."""
    g = rl.sg_bit_graph(n_live, n_vertices)
    src, dst, w, pl, reg = (g[k] for k in ("src", "dst", "w", "place_ids", "regions"))
    vertices = np.unique(np.concatenate([src, dst]))
    sg = pkg.SgGraph(src, dst, w)
    assert sg.live_count() == n_live and len(vertices) == n_vertices
    v = np.repeat(np.array([g["person"], g["place"]], np.int64), n_vertices)
    t = np.tile(vertices, 2)
    for eps, max_it in ((0.01, 0), (0.0, 3)):
        batch = sg.recommend_batch(v, ALPHA, eps, max_it)
        off, ids = batch[0], batch[1]
        seg = np.repeat(np.arange(len(v)), np.diff(off))
        present = np.zeros(len(v), bool)
        present[seg[ids == t[seg]]] = True          # recommend_batch's rows of the request hold its region's vertex
        assert not present[t == v].any()
        for limit in (1, 5):
            want = ranked(mains, batch, pl, reg, t, limit)
            got = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, pl, reg, t, limit)
            st = pkg_stats(sg)
            assert same_all(got, want), (eps, max_it, limit)
            cnt = got[2]
            assert set(cnt.tolist()) == {0, 1} and np.array_equal(cnt == 1, present)
            assert np.array_equal(got[0][cnt == 1, 0], t[cnt == 1])
            assert cnt[t == v].tolist() == [0, 0]                       # the targets' own regions
            assert st["emitted_rows"] == cnt.sum() and st["tiles"] == 1 and st["groups"] == 1
            if max_it == 0:
                assert cnt.sum() == 2 * (n_vertices - 1)
            else:                                                       # the live vertices, all reached; no person
                assert cnt.sum() == 2 * n_live - 1
            if (n_live, n_vertices) == (256, 257):
                monkeypatch.setenv("LOCREC_SG_RANKED_ROW_BUDGET", "64")
                again = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, pl, reg, t, limit)
                groups = pkg_stats(sg)["groups"]
                monkeypatch.delenv("LOCREC_SG_RANKED_ROW_BUDGET")
                assert same_all(again, want) and groups > 1
        check_ends_against_oracle(oracle, src, dst, w, v, t, eps, max_it, pl, reg, 5, got)
    sg.close()


# ---- SG rows into the ranker's other two paths, and the three parity paths of the emit -----------------------------------

# (the sizes and the requests of test_gpu_sg_ranked.test_stats_bound_the_read_back's 3000-place branch; PLACE0 is that
# module's, which its places_table is built on)
N_PERSONS, N_PLACES, N_CATEGORIES = 1_200, 3_000, 20


@pytest.fixture(scope="module")
def world(pkg):
    """The 3000-place world of test_gpu_sg_ranked.test_stats_bound_the_read_back: a region holds about 1000 vertices."""
    from locations_recommender_amd import synth
    g = synth.sg_dataset(n_persons=N_PERSONS, n_places=N_PLACES, n_categories=N_CATEGORIES, seed=8)
    sg = pkg.SgGraph(g["source_id"], g["target_id"], g["balanced_weight"])
    pl, reg = places_table(N_PLACES)
    person0 = int(g["first_person"])
    v = np.r_[person0 + np.arange(0, 1200, 40), PLACE0 + np.arange(0, 3000, 500)].astype(np.int64)
    t = (np.arange(len(v)) % 3).astype(np.int64)
    yield dict(g=g, sg=sg, pl=pl, reg=reg, v=v, t=t, person0=person0)
    sg.close()


def test_other_ranker_paths(pkg, oracle, mains, world, monkeypatch):
    """A region has more than 600 live places here, so the ranked batch's Nd = min(limit, largest region) goes over 256:
    the global radix path from SG at 257, 600 and 2^40, the LDS list at 256.  Then the list with chunks of 64 rows: the
    segments that sg_rk_emit wrote (rows in the order of the atomics, not of the emit rows) through rb_select's chunks
    and rb_merge; and the global path forced for small limits.
    Bites (tried): `N > LOCREC_RANK_BATCH_MAX_N` read as `>=` - 256 is sorted."""
    wd = world
    sg, pl, reg, v, t = wd["sg"], wd["pl"], wd["reg"], wd["v"], wd["t"]
    src, dst, w = wd["g"]["source_id"], wd["g"]["target_id"], wd["g"]["balanced_weight"]
    eps, max_it = 0.01, 20
    largest = int(region_popcounts(wd["g"], pl, reg, t).max())
    assert largest > 600
    batch = sg.recommend_batch(v, ALPHA, eps, max_it)
    wants = {}
    for limit in (256, 257, 600, 2 ** 40):
        wants[limit] = ranked(mains, batch, pl, reg, t, limit)
        got = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, pl, reg, t, limit)
        st = pkg.prep.rank_recommendations_batch_stats()
        assert same_all(got, wants[limit]), limit
        assert (st["sorted"] > 0) == (min(limit, largest) > 256) == (limit > 256), (limit, st)
        if limit > 256:
            assert got[2].max() > 256                       # more rows than the list could have held came back
    check_ends_against_oracle(oracle, src, dst, w, v, t, eps, max_it, pl, reg, 600, sg.recommend_ranked_batch(
        v, ALPHA, eps, max_it, pl, reg, t, 600))
    wants[10] = ranked(mains, batch, pl, reg, t, 10)
    for env, value in (("LOCREC_RANK_BATCH_CHUNK", "64"), ("LOCREC_RANK_BATCH_SORT", "1")):
        for limit in (10, 256):
            monkeypatch.setenv(env, value)
            got = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, pl, reg, t, limit)
            st = pkg.prep.rank_recommendations_batch_stats()
            monkeypatch.delenv(env)
            assert same_all(got, wants[limit]), (env, limit)
            if env == "LOCREC_RANK_BATCH_CHUNK":
                assert st["split"] > 0 and st["sorted"] == 0 and st["chunks"] > 2 * st["split"], st
            else:
                assert st["sorted"] == len(v) and st["split"] == 0, st


def parity_targets(person0):
    """16 distinct targets, a full tile: 8 persons, 6 places, 2 categories.  Chosen on the CPU with oracle.sg_recommend so
    that at (0.01, 20) the columns of the tile stop after odd and after even numbers of sweeps: the persons and the
    categories of this world converge at iteration 2 (their third sweep finds it), the places 40, 290, 790 and 1040 at
    iteration 3, the places 540 and 1290 at 2.  A target's column is its position here, and sg_rk_emit selects the
    columns in pairs (2 k, 2 k + 1): the first four pairs hold one column of each parity, in both orders.  The test
    asserts all of it from the device's own counts."""
    p = person0 + np.arange(0, 1200, 150)
    return np.r_[40, p[0], p[1], 290, 790, p[2], p[3], 1040, p[4:], [540, 1290], [3, 11]].astype(np.int64)


@pytest.mark.parametrize("eps,max_it,kind", [(0.0, 2, "even"), (0.0, 3, "odd"), (0.01, 20, "mixed")])
def test_parity_paths_of_the_emit(oracle, mains, world, eps, max_it, kind):
    """sg_rk_emit reads each column of x from the buffer its last sweep wrote: one load per row when all 16 columns
    stopped after an even number of sweeps, or all after an odd number, two loads and a select per column otherwise.
    The number of sweeps of a column is its iteration count, plus one where it converged (the sweep that found it).
    Bites (tried, one at a time): the one-load branch always reading the first buffer fails "odd" alone; the mixed branch
    taking column 2 k's parity for column 2 k + 1 fails "mixed" alone - with both orders of parity inside a pair, which
    parity_targets arranges."""
    wd = world
    sg, pl, reg = wd["sg"], wd["pl"], wd["reg"]
    src, dst, w = wd["g"]["source_id"], wd["g"]["target_id"], wd["g"]["balanced_weight"]
    v = parity_targets(wd["person0"])
    assert len(v) == len(np.unique(v)) == 16
    t = (np.arange(16) % 3).astype(np.int64)
    want = expected(mains, sg, v, eps, max_it, pl, reg, t, 10)
    got = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, pl, reg, t, 10)
    assert same_all(got, want) and got[2].min() == 10 and pkg_stats(sg)["tiles"] == 1
    its, conv = got[3], got[4]
    sweeps = its + conv
    print(kind, "iterations", its.tolist(), "converged", conv.astype(int).tolist())
    if kind == "even":
        assert not conv.any() and (its % 2 == 0).all() and (sweeps % 2 == 0).all()
    elif kind == "odd":
        assert not conv.any() and (its % 2 == 1).all() and (sweeps % 2 == 1).all()
    else:
        assert conv.all() and (its % 2 == 0).any() and (its % 2 == 1).any()
        assert (sweeps % 2 == 0).any() and (sweeps % 2 == 1).any()
        first, second = sweeps[0::2] % 2, sweeps[1::2] % 2         # the two columns of a pair, both orders of parity
        assert ((first == 0) & (second == 1)).any() and ((first == 1) & (second == 0)).any()
    check_ends_against_oracle(oracle, src, dst, w, v, t, eps, max_it, pl, reg, 10, got)


# ---- ids that look like padding or sit at the ends of int64 --------------------------------------------------------------

def test_extreme_ids(pkg, oracle, mains):
    """Vertex ids I64_MIN, I64_MIN + 1, -1, 0, I64_MAX - 1, I64_MAX and regions I64_MIN, -5, I64_MAX through the whole
    ranked entry: sg_rk_members searches ids and regions in signed order, the ranker behind it by ordered_key.  Every
    vertex is a target, with each of the three regions.  The row whose id is -1 is told from the padding by the count.
    Bites (tried): an unsigned comparison in rk_lower_bound (negative ids and regions are not found)."""
    g = rl.sg_extreme_graph()
    src, dst, w, pl, reg = (g[k] for k in ("src", "dst", "w", "place_ids", "regions"))
    sg = pkg.SgGraph(src, dst, w)
    v = np.repeat(g["vertices"], 3)
    t = np.tile(np.array(rl.EXTREME_REGIONS, np.int64), len(g["vertices"]))
    assert len(v) == 120
    for eps, max_it in ((0.01, 0), (0.0, 5)):
        for limit in (1, 2 ** 40):
            want = expected(mains, sg, v, eps, max_it, pl, reg, t, limit)
            got = sg.recommend_ranked_batch(v, ALPHA, eps, max_it, pl, reg, t, limit)
            assert same_all(got, want), (eps, max_it, limit)
            assert pkg_stats(sg)["tiles"] == 3 and got[2].min() > 0
            if limit > 1:
                returned = set()
                for i in range(len(v)):
                    returned |= set(got[0][i, :got[2][i]].tolist())
                live = set(np.unique(dst).tolist())
                assert returned == (set(g["vertices"].tolist()) if max_it == 0 else live)
                assert set(rl.EXTREME_IDS) & live <= returned
                # -1 as a row: inside the count; -1 as padding: behind it
                i = int(np.flatnonzero((v != -1) & (t == reg[pl == -1][0]))[0])     # -1 is a place of this request's region
                col = int(np.flatnonzero(got[0][i] == -1)[0])
                assert col < got[2][i] and got[1][i, col] > 0
                assert got[2][i] == got[0].shape[1] or (got[0][i, got[2][i]:] == -1).all()
        check_ends_against_oracle(oracle, src, dst, w, v, t, eps, max_it, pl, reg, 2 ** 40, got)
    sg.close()
