"""GPU: locrec_rank_recommendations_batch_by_category (csrc/rank_batch.hip) against existing, unchanged code - the place
table cut to the listings that pass (target region; allow-list; prep.distance_meters(centre, listing) <= radius),
oracle.rank_recommendations at limit = segment length per segment, then the greedy walk with a counter per category
(rank_category_cases.expected).  Nothing is computed, only moved: ids, score bits, distance bits and counts are compared
for equality, on the LDS-list path and on the radix path, with host and with device arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

import rank_batch_cases as rb
import rank_category_cases as rc
import rank_exclude_cases as rx
import rank_near_cases as rn

pytestmark = pytest.mark.gpu
HOST_DEVICE = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
SORT = pytest.mark.parametrize("sort", [False, True], ids=["lists", "sort"])
STATS = ("one_block", "split", "chunks", "sorted")


@pytest.fixture(scope="module")
def prep(pkg):
    return pkg.prep


_WANT, _KEPT = {}, {}


def want(prep, oracle, name, case, limit):
    """The composition of one (case, limit), computed once and shared; the kept rows of a case with circles come from one
    call of the device haversine."""
    key = (name, limit)
    if key not in _WANT:
        if "radius" in case and name not in _KEPT:
            _KEPT[name] = rn.all_kept(prep.distance_meters, case)
        _WANT[key] = rc.expected(oracle.rank_recommendations, case, limit, _KEPT.get(name))
    return _WANT[key]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(x):
    return tuple(a.cpu().numpy() if torch.is_tensor(a) else a for a in x)


def run(prep, case, limit, on_device):
    a, kw = rc.args(case, limit)
    before = [np.array(v, copy=True) for v in a if isinstance(v, np.ndarray)]
    if on_device:
        a = [dev(v) if isinstance(v, np.ndarray) else v for v in a]
        kw = {k: tuple(dev(x) for x in v) if isinstance(v, tuple) else dev(v) for k, v in kw.items()}
    got = host(prep.rank_recommendations_batch_by_category(*a, **kw))
    assert prep.rank_recommendations_batch_stats()["host_syncs"] <= 3
    after = [v.cpu().numpy() if torch.is_tensor(v) else v for v in a if torch.is_tensor(v) or isinstance(v, np.ndarray)]
    assert all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y)
               for x, y in zip(before, after))                                       # the inputs are unchanged
    return got


def check_path(prep, nseg, sort, limit):
    st = prep.rank_recommendations_batch_stats()
    assert st["host_assembled"] == 0
    if sort or limit > 256:
        assert st["sorted"] == nseg and st["one_block"] == 0 and st["split"] == 0
    else:
        assert st["sorted"] == 0 and st["one_block"] + st["split"] == nseg
    return st


@pytest.mark.parametrize("seed", range(4))
@SORT
@HOST_DEVICE
def test_fuzz(prep, oracle, seed, sort, on_device, monkeypatch):
    """Five categories, allow-lists of every kind, a cap per segment out of 1, 2, N - 1, N, N + 1, 2^63 - 1; odd seeds carry
    exclusion lists, seeds 2 and 3 circles of radius 0, 400 m and +inf."""
    if sort:
        monkeypatch.setenv("LOCREC_RANK_BATCH_SORT", "1")
    base = rc.fuzz_case(seed, lists=seed % 2 == 1, circles=seed >= 2)
    nseg = len(base["targets"])
    for limit in rc.LIMITS:
        case = rc.with_caps(base, limit, seed)
        got = run(prep, case, limit, on_device)
        st = check_path(prep, nseg, sort, limit)
        if seed % 2 == 0 and not sort and limit <= 256:
            assert st["split"] >= 1 and st["chunks"] >= 2                             # the 5000-row segment
        assert rc.same(got, want(prep, oracle, ("fuzz", seed, "caps"), case, limit)), limit


@pytest.mark.parametrize("seed", (0, 3))
@SORT
@HOST_DEVICE
def test_lists_without_caps(prep, oracle, seed, sort, on_device, monkeypatch):
    """Every cap NULL, or N and more: the uncapped select with the categories' test."""
    if sort:
        monkeypatch.setenv("LOCREC_RANK_BATCH_SORT", "1")
    base = rc.fuzz_case(seed, lists=seed % 2 == 1, circles=seed >= 2)
    nseg = len(base["targets"])
    for limit in (1, 10, 256, 257):
        w = want(prep, oracle, ("fuzz", seed, "free"), base, limit)
        assert rc.same(run(prep, base, limit, on_device), w), limit
        check_path(prep, nseg, sort, limit)
        loose = dict(base, caps=np.where(np.arange(nseg) % 2 == 0, limit, rc.NO_CAP).astype(np.int64))
        assert rc.same(run(prep, loose, limit, on_device), w), limit


@pytest.mark.parametrize("seed", (0, 1))
@SORT
@HOST_DEVICE
def test_caps_without_lists_and_one_category_per_place(prep, oracle, seed, sort, on_device, monkeypatch):
    if sort:
        monkeypatch.setenv("LOCREC_RANK_BATCH_SORT", "1")
    for few in (True, False):
        base = rc.fuzz_case(seed, few=few, allow=False)
        for limit in (2, 10, 257):
            case = rc.with_caps(base, limit, seed)
            assert rc.same(run(prep, case, limit, on_device), want(prep, oracle, ("nolist", seed, few), case, limit)), (few, limit)


def plain_call(prep, case, limit, on_device):
    """The call a case without categories makes today: plain, excluding or near."""
    d = (lambda v: dev(v)) if on_device else (lambda v: v)
    if "radius" in case:
        a, kw = rn.args(case, limit)
        ids, scores, meters, counts = host(prep.rank_recommendations_batch_near(*[d(v) for v in a[:-1]], a[-1],
                                                                                **{k: d(v) for k, v in kw.items()}))
        return ids, scores, meters, counts
    if "ex_ids" in case:
        a, x = rx.args(case)
        ids, scores, counts = host(prep.rank_recommendations_batch_excluding(*[d(v) for v in a], limit, *[d(v) for v in x]))
    else:
        ids, scores, counts = host(prep.rank_recommendations_batch(*[d(v) for v in rb.args(case)], limit))
    return ids, scores, None, counts


@pytest.mark.parametrize("kind", ["plain", "excluding", "near"])
@SORT
@HOST_DEVICE
def test_identity_is_the_existing_call_bit_for_bit(prep, kind, sort, on_device, monkeypatch):
    """No lists and every cap NULL or N and more: the existing kernels, the existing call's outputs and stats."""
    if sort:
        monkeypatch.setenv("LOCREC_RANK_BATCH_SORT", "1")
    base = rc.fuzz_case(2, lists=kind != "plain", circles=kind == "near", allow=False)
    nseg = len(base["targets"])
    before = plain_call(prep, base, 10, on_device)
    for limit in (1, 10, 256, 257):
        plain = plain_call(prep, base, limit, on_device)
        pst = prep.rank_recommendations_batch_stats()
        for caps in (None, np.full(nseg, max(limit, 1), np.int64), np.full(nseg, rc.NO_CAP, np.int64)):
            case = base if caps is None else dict(base, caps=caps)
            got = run(prep, case, limit, on_device)
            st = prep.rank_recommendations_batch_stats()
            assert rc.same(got, plain, meters=kind == "near"), limit
            assert [st[k] for k in STATS] == [pst[k] for k in STATS] and st["host_syncs"] == pst["host_syncs"]
        # lists given, all of them empty: the same
        empty = rc.with_allow(base, [np.empty(0, np.int64)] * nseg)
        assert rc.same(run(prep, empty, limit, on_device), plain, meters=kind == "near")
    # afterwards the plain call returns what it returned before
    assert rc.same(plain_call(prep, base, 10, on_device), before, meters=kind == "near")


@SORT
@HOST_DEVICE
def test_dominant_category(prep, oracle, sort, on_device, monkeypatch):
    if sort:
        monkeypatch.setenv("LOCREC_RANK_BATCH_SORT", "1")
    case = rc.dominant_case()
    ids, scores, _, counts = got = run(prep, case, rc.DOMINANT_N, on_device)
    assert rc.same(got, want(prep, oracle, "dominant", case, rc.DOMINANT_N))
    assert counts.tolist() == [4] and case["cats"][np.searchsorted(case["place_ids"], ids[0])].tolist() == [5, 5, 6, 6]


@pytest.mark.parametrize("n_cats", [1, 3])
@pytest.mark.parametrize("chunk", [None, 64, 1000])
@HOST_DEVICE
def test_ascending_scores(prep, oracle, n_cats, chunk, on_device, monkeypatch):
    """Every compaction's survivors are killed by the rows behind them: one block's buffer compacts six times over 5000
    rows, and with chunks the merge sees partial lists none of whose rows but the last chunk's survive."""
    if chunk:
        monkeypatch.setenv("LOCREC_RANK_BATCH_CHUNK", str(chunk))
    case = rc.ascending_case(n_cats=n_cats)
    for limit in (1, 10, 256):
        got = run(prep, case, limit, on_device)
        st = prep.rank_recommendations_batch_stats()
        assert st["split"] == (1 if (chunk or 4096) < 5000 else 0) and st["chunks"] == (-(-5000 // (chunk or 4096)) if st["split"] else 0)
        assert rc.same(got, want(prep, oracle, ("ascending", n_cats), case, limit)), limit
        assert got[0][0, :got[3][0]].tolist() == list(range(5000, 5000 - min(limit, 2 * n_cats), -1))


@pytest.mark.parametrize("chunks", rb.SEAM_CHUNKS)
@HOST_DEVICE
def test_chunk_seam_with_two_interleaved_categories(prep, oracle, chunks, on_device, monkeypatch):
    monkeypatch.setenv("LOCREC_RANK_BATCH_CHUNK", "64")
    for cap in (1, 3):
        case = rc.seam_case(chunks, cap)
        for limit in rb.SEAM_LIMITS:
            got = run(prep, case, limit, on_device)
            st = prep.rank_recommendations_batch_stats()
            assert st["split"] == 1 and st["chunks"] == chunks + 1 and st["sorted"] == 0
            assert rc.same(got, want(prep, oracle, ("seam", chunks, cap), case, limit)), (cap, limit)


def near_listing_case():
    """One segment over region 4, centre on place 10: place 12 is listed first far away under category 70 and then near
    under 80; place 13 near under 70 and then, nearer, under 80; place 14 near, category 90."""
    place_ids = np.array([10, 11, 12, 12, 13, 13, 14], np.int64)
    lat = np.array([48.8600, 48.8610, 48.9500, 48.8605, 48.8602, 48.8601, 48.8601])
    lon = np.array([2.3100, 2.3110, 2.4000, 2.3102, 2.3101, 2.3100, 2.3099])
    return dict(offsets=np.array([0, 5], np.int64), ids=np.array([10, 11, 12, 13, 14], np.int64),
                scores=np.array([1.0, 2.0, 3.0, 4.0, 5.0]), place_ids=place_ids, regions=np.full(7, 4, np.int64),
                targets=np.array([4], np.int64), cats=np.array([70, 70, 70, 80, 70, 80, 90], np.int64), lat=lat, lon=lon,
                clat=np.array([48.8600]), clon=np.array([2.3100]), radius=np.array([100.0]))


@SORT
@HOST_DEVICE
def test_the_listing_that_counts(prep, oracle, sort, on_device, monkeypatch):
    if sort:
        monkeypatch.setenv("LOCREC_RANK_BATCH_SORT", "1")
    case = rc.listing_case()
    ids, _, meters, counts = got = run(prep, case, 5, on_device)
    assert meters is None and rc.same(got, want(prep, oracle, "listing", case, 5))
    for s, expect in enumerate(rc.LISTING_IDS):
        assert ids[s, :counts[s]].tolist() == expect, s
    # with a circle: out_meters is the distance of the listing that counts under all three predicates
    near = near_listing_case()
    dist = prep.distance_meters(np.full(7, near["clat"][0]), np.full(7, near["clon"][0]), near["lat"], near["lon"])
    ids, _, meters, counts = got = run(prep, near, 5, on_device)                      # no list: 11 (133 m) is outside
    assert rc.same(got, want(prep, oracle, "near listing", near, 5))
    assert ids[0, :counts[0]].tolist() == [14, 13, 12, 10]
    assert meters[0, :4].tobytes() == dist[[6, 4, 3, 0]].tobytes()                    # 13: its first listing, 12: its second
    only80 = rc.with_allow(near, [np.array([80], np.int64)])
    ids, _, meters, counts = got = run(prep, only80, 5, on_device)
    assert rc.same(got, want(prep, oracle, "near listing 80", only80, 5))
    assert ids[0, :counts[0]].tolist() == [13, 12] and meters[0, :2].tobytes() == dist[[5, 3]].tobytes()
    capped = dict(near, caps=np.array([1], np.int64))                                 # 14 (90), 13 (70), 12 (80); 10 is a second 70
    ids, _, meters, counts = got = run(prep, capped, 5, on_device)
    assert rc.same(got, want(prep, oracle, "near listing cap", capped, 5))
    assert ids[0, :counts[0]].tolist() == [14, 13, 12] and meters[0, :3].tobytes() == dist[[6, 4, 3]].tobytes()


@HOST_DEVICE
def test_edges(prep, on_device):
    """Segments of 0 rows, a target region with no place, no places, no segments, max_recommendations <= 0."""
    base = rc.with_caps(rc.fuzz_case(3, circles=True), 5)
    nseg = len(base["targets"])
    ids, _, meters, cnt = run(prep, base, 5, on_device)
    empty = (np.diff(base["offsets"]) == 0) | (base["targets"] == 99)
    assert empty.any() and not cnt[empty].any() and (ids[empty] == -1).all() and not meters[empty].any()
    for limit in (0, -1):
        ids, scores, meters, cnt = run(prep, base, limit, on_device)
        assert ids.shape == meters.shape == (nseg, 0) and not cnt.any()
    none = np.empty(0, np.int64)
    case = dict(base, place_ids=none, regions=none, cats=none, lat=np.empty(0), lon=np.empty(0))
    got = run(prep, case, 5, on_device)
    assert not got[3].any() and got[0].shape == (nseg, 5) and (got[0] == -1).all() and not got[2].any()
    case = dict(base, offsets=np.zeros(1, np.int64), targets=none, clat=np.empty(0), clon=np.empty(0), radius=np.empty(0),
                caps=none, al_offsets=np.zeros(1, np.int64), al_ids=none)
    assert run(prep, case, 5, on_device)[3].shape == (0,)


@pytest.mark.parametrize("limit", [4, 0])
@pytest.mark.parametrize("bad", ["cap", "offsets", "radius"])
def test_device_arrays_are_refused_in_the_plan_step(pkg, bad, limit):
    """Device arrays are checked on the device, before any row is read, and nothing is written."""
    from locations_recommender_amd import _lib as L
    case = near_listing_case()
    case.update(al_offsets=np.array([0, 1], np.int64), al_ids=np.array([80, 70], np.int64), caps=np.array([1], np.int64))
    if bad == "cap":
        case["caps"] = np.array([0], np.int64)
    elif bad == "offsets":
        case["al_offsets"] = np.array([0, 3], np.int64)
    else:
        case["radius"] = np.array([-1.0])
    keys = ("offsets", "ids", "scores", "place_ids", "regions", "lat", "lon", "cats", "targets", "clat", "clon", "radius", "al_offsets",
            "al_ids", "caps")
    a = {k: dev(case[k]) for k in keys}
    a.update(oi=dev(np.full(4, 77, np.int64)), osc=dev(np.full(4, 7.5)), om=dev(np.full(4, 7.5)), oc=dev(np.full(1, 77, np.int64)))
    torch.cuda.synchronize()
    p = {k: C.c_void_p(v.data_ptr()) for k, v in a.items()}
    rc_ = L.lib().locrec_rank_recommendations_batch_by_category(
        1, p["offsets"], 5, p["ids"], p["scores"], 7, p["place_ids"], p["regions"], p["lat"], p["lon"], p["cats"], p["targets"],
        p["clat"], p["clon"], p["radius"], limit, None, 0, None, p["al_offsets"], 2, p["al_ids"], p["caps"], L.MEM_DEVICE,
        p["oi"], p["osc"], p["om"], p["oc"])
    assert rc_ == L.E_INVALID_ARG
    word = {"cap": b"max_per_category", "offsets": b"allowed_offsets", "radius": b"radius_meters"}[bad]
    assert word in L.lib().locrec_last_error()
    oi, osc, om, oc = host((a["oi"], a["osc"], a["om"], a["oc"]))
    assert (oi == 77).all() and (osc == 7.5).all() and (om == 7.5).all() and (oc == 77).all()
    assert pkg.prep.rank_recommendations_batch_stats()["host_syncs"] <= 3
