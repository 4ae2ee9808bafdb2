"""GPU checks of the region sets of the builder mains (csrc/region_sets.hip, prep.RegionSetPlan and the builder mains'
bodies in mains.py) against the numpy restatement of tests/region_set_cases.py.  Every comparison is integer equality
(float64 columns are compared as their int64 bit patterns)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import region_set_cases as rsc

pytestmark = pytest.mark.gpu
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
SENTINEL = -777


@pytest.fixture(scope="module")
def prep(pkg):
    return pkg.prep


@pytest.fixture(scope="module")
def L(pkg):
    from locations_recommender_amd import _lib
    return _lib


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def dev_table(table):
    return {k: dev(v) for k, v in table.items()}


def assert_same_visits(got, want, what=None):
    assert sorted(got) == sorted(rsc.PLACE_VISIT_COLUMNS), what
    for k in rsc.PLACE_VISIT_COLUMNS:
        g = host(got[k])
        assert g.dtype == np.int64 and np.array_equal(g, want[k]), (what, k)


# ---- max(timestamp) and the distinct region ids ------------------------------------------------------------------------

ID_CASES = {
    "duplicates": np.array([5, 3, 5, 5, 3, 9, 3], np.int64),
    "negative": np.array([-1, -50, 7, -1, 0, -50, 7], np.int64),
    "limits": np.array([I64_MAX, 0, I64_MIN, -1, I64_MAX, I64_MIN, 1], np.int64),
    "one": np.array([-42], np.int64),
    "many": np.random.default_rng(1).integers(-300, 300, 100_003),
}


@pytest.mark.parametrize("name", sorted(ID_CASES))
@pytest.mark.parametrize("on_device", [False, True])
def test_extract_region_ids_and_max_timestamp(prep, name, on_device):
    a = ID_CASES[name]
    x = dev(a) if on_device else a
    got = prep.extract_region_ids(x)
    assert torch.is_tensor(got) == on_device
    assert host(got).dtype == np.int64 and np.array_equal(host(got), rsc.extract_region_ids(a))
    assert prep.max_timestamp(x) == rsc.max_timestamp(a)


@pytest.mark.parametrize("on_device", [False, True])
def test_no_rows(prep, pkg, on_device):
    none = dev(np.empty(0, np.int64)) if on_device else np.empty(0, np.int64)
    assert len(prep.extract_region_ids(none)) == 0
    with pytest.raises(pkg.IllegalArgumentException):
        prep.max_timestamp(none)


@pytest.mark.parametrize("on_device", [False, True])
def test_extract_region_ids_capacity_below_the_count(L, on_device):
    """Count only with a NULL output; a capacity below the count gets the first `capacity` ids and the true count, and
    the entries behind the capacity stay as they were."""
    a = ID_CASES["limits"]
    want = rsc.extract_region_ids(a)
    src = dev(a) if on_device else a
    srcp = C.c_void_p(src.data_ptr() if on_device else src.ctypes.data)
    mem = L.MEM_DEVICE if on_device else L.MEM_HOST
    cnt = C.c_int64(123)
    L.check(L.lib().locrec_extract_region_ids(len(a), srcp, mem, None, C.byref(cnt)))
    assert cnt.value == len(want) == 5
    for cap in (0, 1, 3, 5, 8):
        out = np.full(8, SENTINEL, np.int64)
        o = dev(out) if on_device else out
        cnt = C.c_int64(cap)
        L.check(L.lib().locrec_extract_region_ids(len(a), srcp, mem, C.c_void_p(o.data_ptr() if on_device else o.ctypes.data),
                                                  C.byref(cnt)))
        m = min(cap, len(want))
        assert cnt.value == len(want)
        assert np.array_equal(host(o)[:m], want[:m]) and np.all(host(o)[m:] == SENTINEL), cap


# ---- the partition and the gather at the limits of the merge's tile -------------------------------------------------

def check_plan(prep, table, listed, on_device, what):
    regions = table["region_id"]
    plan = prep.RegionSetPlan(dev_table(table) if on_device else table, listed[::-1])   # any order in
    rows, offsets = rsc.partition(regions, np.sort(listed))
    assert plan.region_ids == np.sort(listed).tolist()
    assert plan.offsets == offsets.tolist(), what
    assert host(plan.rows).dtype == np.int32 and np.array_equal(host(plan.rows)[:len(rows)], rows), what
    for rs in rsc.region_sets(listed):
        want = rsc.place_visits_of_set(table, rs)
        assert plan.count(rs) == len(want["person_id"])
        got = plan.place_visits(rs)
        assert torch.is_tensor(got["person_id"]) == on_device
        assert_same_visits(got, want, (what, rs))
        assert_same_visits(plan.place_visits(rs[::-1]), want, (what, rs, "swapped"))
    return plan


@pytest.mark.parametrize("how", rsc.INTERLEAVINGS)
@pytest.mark.parametrize("la,lb", rsc.RUN_LENGTHS)
def test_partition_and_gather_at_the_tile_limits(prep, la, lb, how):
    regions, listed = rsc.run_case(la, lb, how, seed=la * 3 + lb)
    table = rsc.table_for(regions, seed=lb)
    plan = check_plan(prep, table, listed, True, (la, lb, how))
    assert plan.count((rsc.REGION_A,)) == la and plan.count((rsc.REGION_B,)) == lb and plan.count((rsc.REGION_EMPTY,)) == 0
    assert plan.offsets[-1] - plan.offsets[-2] == (regions == rsc.REGION_UNLISTED).sum() >= 2
    assert len(plan.place_visits((rsc.REGION_EMPTY,))["person_id"]) == 0


def test_seven_regions_on_seventy_thousand_rows(prep):
    regions, ids = rsc.many_regions_case(3)
    plan = check_plan(prep, rsc.table_for(regions, seed=1), ids, True, "R=7")
    assert len(rsc.region_sets(ids)) == 28 == len(prep.region_sets(plan.region_ids))


@pytest.mark.parametrize("la,lb,how", [(2049, 2047, "random"), (1, 1, "alternating"), (4097, 3, "b_first"), (0, 0, "random")])
def test_host_and_device_memory_give_equal_results(prep, la, lb, how):
    regions, listed = rsc.run_case(la, lb, how, seed=5)
    table = rsc.table_for(regions, seed=6)
    ph = check_plan(prep, table, listed, False, (la, lb, how, "host"))
    pd = check_plan(prep, table, listed, True, (la, lb, how, "device"))
    assert ph.offsets == pd.offsets and np.array_equal(ph.rows[:ph.n], host(pd.rows)[:pd.n])
    for rs in rsc.region_sets(listed):
        h, d = ph.place_visits(rs), pd.place_visits(rs)
        for k in rsc.PLACE_VISIT_COLUMNS:
            assert np.array_equal(h[k], host(d[k])), (rs, k)


def test_plan_without_rows_and_with_one_region(prep, pkg):
    empty = {k: np.empty(0, np.int64) for k in rsc.PLACE_VISIT_COLUMNS}
    for on_device in (False, True):
        plan = prep.RegionSetPlan(dev_table(empty) if on_device else empty, [4, 2, 9])
        assert plan.offsets == [0] * 5
        assert all(len(v) == 0 for v in plan.place_visits((2, 9)).values())
        one = rsc.table_for(np.array([8, 8, 1, 8], np.int64))
        plan = prep.RegionSetPlan(dev_table(one) if on_device else one, [8])
        assert plan.offsets == [0, 3, 4] and host(plan.rows)[:4].tolist() == [0, 1, 3, 2]
        assert host(plan.place_visits((8,))["person_id"]).tolist() == [2040, 2047, 2061]
        with pytest.raises(pkg.IllegalArgumentException):
            plan.place_visits((1,))                      # not one of the plan's regions
        with pytest.raises(pkg.IllegalArgumentException):
            prep.RegionSetPlan(dev_table(one) if on_device else one, [8, 8])


# ---- the refusals ------------------------------------------------------------------------------------------------------

def raw_gather(L, on_device, n_rows, cols, rows, a0, a1, b0, b1, out_len):
    """locrec_region_set_gather on raw arrays -> (status, outputs as numpy); the outputs are pre-filled with SENTINEL."""
    mem = L.MEM_DEVICE if on_device else L.MEM_HOST
    keep = [dev(c) if on_device else np.ascontiguousarray(c, np.int64) for c in cols]
    r = dev(np.asarray(rows, np.int32)) if on_device else np.ascontiguousarray(rows, np.int32)
    outs = [dev(np.full(out_len, SENTINEL, np.int64)) if on_device else np.full(out_len, SENTINEL, np.int64) for _ in cols]
    p = (lambda a: a.data_ptr()) if on_device else (lambda a: a.ctypes.data)
    cin, cout = (C.c_void_p * len(cols))(*[p(a) for a in keep]), (C.c_void_p * len(cols))(*[p(a) for a in outs])
    status = L.lib().locrec_region_set_gather(n_rows, len(cols), cin, C.c_void_p(p(r)), a0, a1, b0, b1, mem, cout)
    if on_device:
        torch.cuda.synchronize()
    return status, [host(o) for o in outs]


@pytest.mark.parametrize("on_device", [False, True])
def test_gather_refuses_bad_rows_and_writes_nothing(L, on_device):
    n = 6000
    cols = [np.arange(n, dtype=np.int64) * 3, np.arange(n, dtype=np.int64) - 9]
    good = np.arange(n, dtype=np.int32)
    status, outs = raw_gather(L, on_device, n, cols, good, 0, 2500, 2500, 5000, 5000)   # the good call, for contrast
    assert status == L.OK and np.array_equal(outs[0], cols[0][:5000]) and np.array_equal(outs[1], cols[1][:5000])
    # two columns' worth of an interleaved merge: evens then odds
    rows = np.r_[np.arange(0, n, 2), np.arange(1, n, 2)].astype(np.int32)
    status, outs = raw_gather(L, on_device, n, cols, rows, 0, 3000, 3000, 6000, 6000)
    assert status == L.OK and np.array_equal(outs[0], cols[0])
    bad = {}
    r = good.copy()
    r[4100], r[4101] = r[4101], r[4100]
    bad["a descending step in the second run"] = (r, 0, 2500, 2500, 5000)
    r = good.copy()
    r[7] = r[6]
    bad["an equal step in the first run"] = (r, 0, 2500, 2500, 5000)
    r = good.copy()
    r[4999] = n
    bad["an index == n_rows"] = (r, 0, 2500, 2500, 5000)
    r = good.copy()
    r[0] = -1
    bad["a negative index"] = (r, 0, 2500, 2500, 5000)
    bad["overlapping ranges"] = (good, 0, 2500, 2499, 5000)
    bad["a range inside the other"] = (good, 0, 5000, 10, 20)
    bad["a range behind the rows"] = (good, 0, 2500, 2500, n + 1)
    bad["a range that runs backwards"] = (good, 30, 20, 2500, 5000)
    for what, (r, a0, a1, b0, b1) in bad.items():
        status, outs = raw_gather(L, on_device, n, cols, r, a0, a1, b0, b1, 6000)
        assert status == L.E_INVALID_ARG, what
        assert all(np.all(o == SENTINEL) for o in outs), what
    status, _ = raw_gather(L, on_device, n, cols[:1] * 9, good, 0, 10, 10, 20, 20)
    assert status == L.E_INVALID_ARG                       # more than 8 columns


@pytest.mark.parametrize("on_device", [False, True])
def test_partition_refuses_unsorted_region_ids_and_writes_nothing(L, on_device):
    mem = L.MEM_DEVICE if on_device else L.MEM_HOST
    regions = np.array([3, 5, 3, 7, 5, 5], np.int64)
    rr = dev(regions) if on_device else regions
    p = (lambda a: a.data_ptr()) if on_device else (lambda a: a.ctypes.data)
    for listed in ([5, 3, 7], [3, 5, 5], [3, 7, 5]):
        ids = dev(np.asarray(listed, np.int64)) if on_device else np.asarray(listed, np.int64)
        rows = np.full(6, SENTINEL, np.int32)
        out = dev(rows) if on_device else rows
        offsets = (C.c_int64 * 5)(*[SENTINEL] * 5)
        status = L.lib().locrec_region_partition(6, C.c_void_p(p(rr)), 3, C.c_void_p(p(ids)), mem, C.c_void_p(p(out)), offsets)
        assert status == L.E_INVALID_ARG, listed
        assert np.all(host(out) == SENTINEL) and list(offsets) == [SENTINEL] * 5, listed
    offsets = (C.c_int64 * 5)()
    assert L.lib().locrec_region_partition(-1, None, 3, None, mem, None, offsets) == L.E_INVALID_ARG
    assert L.lib().locrec_region_partition(1 << 31, C.c_void_p(p(rr)), 0, None, mem, C.c_void_p(p(rr)), offsets) == L.E_INVALID_ARG


# ---- end to end: the plan's visits build the same graphs and indexes as numpy-filtered visits --------------------------

@pytest.fixture(scope="module")
def builder_tables(prep):
    """The two sample tables of a 3-region case, their place visits on the device and on the host, and the regions."""
    visits, places, visits_from = rsc.builder_case()
    pv = prep.calc_place_visits(dev_table(visits), dev_table(places), visits_from)
    pv_host = {k: host(v) for k, v in pv.items()}
    regions = host(prep.extract_region_ids(dev(places["region_id"]))).tolist()
    assert regions == [-5, 2, 9] and 200 <= len(pv_host["person_id"]) <= 2000
    return visits, places, visits_from, pv, pv_host, regions


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_plan_visits_give_the_same_graph_edges(prep, builder_tables):
    _, _, _, pv, pv_host, regions = builder_tables
    plan = prep.RegionSetPlan(pv, regions)
    sets = prep.region_sets(regions)
    assert len(sets) == 6
    for rs in sets:
        want_pv = rsc.place_visits_of_set(pv_host, rs)
        assert len(want_pv["person_id"]) > 0
        assert_same_visits(plan.place_visits(rs), want_pv, rs)
        got = prep.generate_stochastic_graph(plan.place_visits(rs), 0.7, 0.3)
        want = prep.generate_stochastic_graph(dev_table(want_pv), 0.7, 0.3)
        assert len(host(got[0])) > 0
        for g, w in zip(got, want):
            assert same_bits(g, w), rs


def test_plan_visits_give_the_same_knn_index(prep, builder_tables):
    _, _, _, pv, pv_host, regions = builder_tables
    built = list(prep.knn_indexes_by_region_set(pv, regions, 100, 10))
    assert [rs for rs, _ in built] == prep.region_sets(regions)
    for rs, ix in built:
        want_pv = dev_table(rsc.place_visits_of_set(pv_host, rs))
        ref = prep.knn_index_from_visits(want_pv["person_id"], want_pv["place_id"], want_pv["category_id"], 100, 10)
        persons = np.unique(host(want_pv["person_id"]))[:8]
        assert len(persons) == 8
        for pid in persons.tolist():
            for g, w in zip(ix.recommend(pid, 0.6, 0.4, 5), ref.recommend(pid, 0.6, 0.4, 5)):
                assert same_bits(g, w), (rs, pid)
            for g, w in zip(ix.query(pid, 0.6, 0.4, 5), ref.query(pid, 0.6, 0.4, 5)):
                assert same_bits(g, w), (rs, pid)
        ix.close()
        ref.close()


def test_sets_without_visits_yield_no_handle(prep, builder_tables):
    _, _, _, pv, _, regions = builder_tables
    listed = regions + [500]                                   # a region of the places that nobody visited
    knn = dict(prep.knn_indexes_by_region_set(pv, listed))
    sg = dict(prep.sg_graphs_by_region_set(prep.RegionSetPlan(pv, listed), listed, 1.0, 1.0))
    assert list(knn) == list(sg) == prep.region_sets(listed) and len(knn) == 10
    for rs in knn:
        if rs == (500,):
            assert knn[rs] is None and sg[rs] is None
        else:
            assert knn[rs] is not None and sg[rs] is not None
            knn[rs].close()
            sg[rs].close()


# ---- the builder mains -------------------------------------------------------------------------------------------------

def write_sample_tables(data_dir, visits, places):
    """location_visits_sample / places_sample as the reference's generator leaves them: a timestamp column, region_id int32."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    pq.write_table(pa.table({"person_id": pa.array(visits["person_id"], pa.int64()),
                             "timestamp": pa.array(visits["timestamp"], pa.int64()).cast(pa.timestamp("ms")),
                             "latitude": visits["latitude"], "longitude": visits["longitude"],
                             "region_id": pa.array(visits["region_id"], pa.int32())}), os.path.join(data_dir, "location_visits_sample"))
    pq.write_table(pa.table({"id": pa.array(places["id"], pa.int64()), "latitude": places["latitude"], "longitude": places["longitude"],
                             "region_id": pa.array(places["region_id"], pa.int32()),
                             "category_id": pa.array(places["category_id"], pa.int64())}), os.path.join(data_dir, "places_sample"))


def native_parquet():
    from locations_recommender_amd import parquet
    return parquet if os.path.exists(parquet.LIB_PATH) else None


def test_rating_vectors_builder_main(prep, pkg, builder_tables, tmp_path):
    from locations_recommender_amd import mains
    visits, places, visits_from, pv, pv_host, regions = builder_tables
    d = str(tmp_path)
    write_sample_tables(d, visits, places)
    assert prep.visits_from_timestamp(int(visits["timestamp"].max()), 60) == visits_from
    written = mains.rating_vectors_builder_main(d, 60, 7, 3)
    assert written == prep.region_sets(regions)
    assert_same_visits(mains.load_place_visits(os.path.join(d, "place_visits")), pv_host)
    direct = dict(prep.knn_indexes_by_region_set(pv, regions, 7, 3))
    for rs in written:
        names = [mains.generate_file_name(rs, d, f) for f in ("place_rating_vectors", "category_rating_vectors", "place_ratings")]
        set_pv = rsc.place_visits_of_set(pv_host, rs)
        pr = mains.calc_ratings(set_pv["person_id"], set_pv["place_id"], 7)
        cr = mains.calc_ratings(set_pv["person_id"], set_pv["category_id"], 3)
        for g, w in zip(mains.load_place_ratings(names[2]), pr):
            assert np.array_equal(g, w), rs
        for name, ratings in ((names[0], pr), (names[1], cr)):
            want = mains.calc_rating_vectors(*ratings)
            got = mains.load_rating_vectors(name)
            assert got[4] == want[4], rs
            for g, w in zip(got[:4], want[:4]):
                assert g.dtype == w.dtype and np.array_equal(g, w), rs
        served = [mains.knn_index_from_parquet(d, rs)]
        if native_parquet() is not None:
            served.append(native_parquet().knn_index(*names))
        persons = np.unique(set_pv["person_id"])[:8]
        for pid in persons.tolist():
            want = direct[rs].recommend(pid, 0.5, 0.5, 6), direct[rs].query(pid, 0.5, 0.5, 6)
            for ix in served:
                got = ix.recommend(pid, 0.5, 0.5, 6), ix.query(pid, 0.5, 0.5, 6)
                for gg, ww in zip(got, want):
                    for g, w in zip(gg, ww):
                        assert same_bits(g, w), (rs, pid)
        for ix in served + [direct[rs]]:
            ix.close()


def test_stochastic_graph_builder_main(prep, pkg, builder_tables, tmp_path):
    import edge_cases
    from locations_recommender_amd import mains
    visits, places, visits_from, pv, pv_host, regions = builder_tables
    d = str(tmp_path)
    write_sample_tables(d, visits, places)
    written = mains.stochastic_graph_builder_main(d, 60, 0.7, 0.3)
    assert written == prep.region_sets(regions)
    assert_same_visits(mains.load_place_visits(os.path.join(d, "place_visits")), pv_host)
    direct = dict(prep.sg_graphs_by_region_set(pv, regions, 0.7, 0.3))
    for rs in written:
        name = mains.generate_file_name(rs, d, "stochastic_graph")
        set_pv = rsc.place_visits_of_set(pv_host, rs)
        want = mains.build_with_balanced_weights([1.0, 1.0, 0.7, 0.3], edge_cases.stochastic_graph_families(set_pv))
        got = mains.load_stochastic_graph(name)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and same_bits(got[2], want[2]), rs
        served = [mains.sg_graph_from_parquet(d, rs)]
        if native_parquet() is not None:
            served.append(native_parquet().sg_graph(name))
        for v in np.unique(set_pv["person_id"])[:3].tolist():
            wi, wp, wit, wconv = direct[rs].recommend(v, 0.15, 0.01, 20)
            for g in served:
                gi, gp, it, conv = g.recommend(v, 0.15, 0.01, 20)
                assert np.array_equal(gi, wi) and same_bits(gp, wp) and (it, conv) == (wit, wconv), (rs, v)
        for g in served + [direct[rs]]:
            g.close()
