"""GPU: locrec_rank_recommendations_batch (csrc/rank_batch.hip) against existing, unchanged code applied per segment -
oracle.rank_recommendations, cross-checked with the single device ranker locrec_rank_recommendations.  Nothing is
computed, only moved: ids, score bits and counts are compared for equality, on host and on device memory."""
import ctypes as C

import numpy as np
import pytest
import torch

import rank_batch_cases as rb

pytestmark = pytest.mark.gpu
HOST_DEVICE = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])


@pytest.fixture(scope="module")
def prep(pkg):
    return pkg.prep


@pytest.fixture(scope="module")
def max_n(pkg):
    from locations_recommender_amd import _lib
    return _lib.RANK_BATCH_MAX_N


_WANT = {}


def want(oracle, name, case, limit):
    """The oracle loop of one (case, limit): computed once, shared by the tests that need it."""
    key = (name, limit)
    if key not in _WANT:
        _WANT[key] = rb.expected(oracle.rank_recommendations, case, limit)
    return _WANT[key]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(x):
    return tuple(a.cpu().numpy() if torch.is_tensor(a) else a for a in x)


def run(prep, case, limit, on_device):
    a = rb.args(case)
    return host(prep.rank_recommendations_batch(*([dev(x) for x in a] if on_device else a), limit))


@pytest.mark.parametrize("seed", range(8))
@HOST_DEVICE
def test_fuzz(prep, oracle, max_n, seed, on_device):
    case = rb.fuzz_case(seed)
    for limit in rb.fuzz_limits(max_n):
        got = run(prep, case, limit, on_device)
        st = prep.rank_recommendations_batch_stats()
        assert rb.same(got, want(oracle, ("fuzz", seed), case, limit)), limit
        assert st["host_syncs"] <= 3 and st["host_assembled"] == 0 and st["membership_form"] == 0
        nseg = len(case["targets"])
        if limit > max_n:
            assert st["sorted"] == nseg and st["one_block"] == 0
        elif limit > 0:
            assert st["sorted"] == 0 and st["one_block"] + st["split"] == nseg
            assert (st["split"] > 0) == bool((np.diff(case["offsets"])[np.isin(case["targets"], (0, 1, 2))] > 4096).any())


@pytest.mark.parametrize("seed", (0, 1))
def test_fuzz_equals_the_single_device_ranker(prep, max_n, seed):
    case = rb.fuzz_case(seed)
    for limit in (2, 10, max_n + 1):
        assert rb.same(run(prep, case, limit, True), rb.expected(prep.rank_recommendations, case, limit)), limit


@pytest.mark.parametrize("seed", range(8))
def test_global_path_reproduces_the_fuzz(prep, oracle, max_n, seed, monkeypatch):
    case = rb.fuzz_case(seed)
    monkeypatch.setenv("LOCREC_RANK_BATCH_SORT", "1")
    for limit in rb.fuzz_limits(max_n):
        got = run(prep, case, limit, True)
        st = prep.rank_recommendations_batch_stats()
        assert rb.same(got, want(oracle, ("fuzz", seed), case, limit)), limit
        if limit > 0:
            assert st["sorted"] == len(case["targets"]) and st["one_block"] == st["split"] == st["chunks"] == 0


@pytest.mark.parametrize("chunks", rb.SEAM_CHUNKS)
@HOST_DEVICE
def test_chunk_seam(prep, oracle, chunks, on_device, monkeypatch):
    case = rb.seam_case(chunks)
    for limit in rb.SEAM_LIMITS:
        monkeypatch.setenv("LOCREC_RANK_BATCH_CHUNK", "64")
        got = run(prep, case, limit, on_device)
        st = prep.rank_recommendations_batch_stats()
        assert rb.same(got, want(oracle, ("seam", chunks), case, limit)), limit
        assert st["split"] == 1 and st["chunks"] == chunks + 1 and st["one_block"] == 0 and st["sorted"] == 0
        monkeypatch.delenv("LOCREC_RANK_BATCH_CHUNK")
        got = run(prep, case, limit, on_device)
        st = prep.rank_recommendations_batch_stats()
        assert rb.same(got, want(oracle, ("seam", chunks), case, limit)), limit
        assert st["split"] == 0 and st["chunks"] == 0 and st["one_block"] == 1


@HOST_DEVICE
def test_small_chunks_on_a_fuzz_case(prep, oracle, max_n, on_device, monkeypatch):
    case = rb.fuzz_case(2)
    monkeypatch.setenv("LOCREC_RANK_BATCH_CHUNK", "64")
    for limit in (1, 10, max_n):
        got = run(prep, case, limit, on_device)
        assert rb.same(got, want(oracle, ("fuzz", 2), case, limit)), limit
        assert prep.rank_recommendations_batch_stats()["split"] > 0


@HOST_DEVICE
def test_extremes(prep, oracle, max_n, on_device):
    case = rb.extremes_case()
    for limit in (1, 3, 10, max_n + 1):
        assert rb.same(run(prep, case, limit, on_device), want(oracle, "extremes", case, limit)), limit


@HOST_DEVICE
def test_edges(prep, oracle, on_device):
    base = rb.fuzz_case(1)
    # every segment empty
    case = dict(base, offsets=np.full(4, 7, np.int64), targets=np.array([0, 1, 2], np.int64))
    ids, scores, cnt = run(prep, case, 5, on_device)
    assert ids.shape == (3, 0) and cnt.tolist() == [0, 0, 0]
    # every row dropped by the join
    case = dict(base, targets=np.full(len(base["targets"]), 99, np.int64))
    got = run(prep, case, 5, on_device)
    assert rb.same(got, rb.expected(oracle.rank_recommendations, case, 5)) and not got[2].any() and (got[0] == -1).all()
    assert not got[1].view(np.uint64).any()
    # no segments; no places
    case = dict(base, offsets=np.zeros(1, np.int64), targets=np.empty(0, np.int64))
    assert run(prep, case, 5, on_device)[2].shape == (0,)
    case = dict(base, place_ids=np.empty(0, np.int64), regions=np.empty(0, np.int64))
    got = run(prep, case, 5, on_device)
    assert not got[2].any() and (got[0] == -1).all() and got[0].shape == (len(base["targets"]), 5)
    # rows outside the segments are ignored
    off = base["offsets"]
    case = dict(base, offsets=off[1:-1].copy(), targets=base["targets"][1:-1].copy())
    assert case["offsets"][0] > 0 and case["offsets"][-1] < len(base["ids"])
    assert rb.same(run(prep, case, 10, on_device), rb.expected(oracle.rank_recommendations, case, 10))


@HOST_DEVICE
@pytest.mark.parametrize("bad", ["decreasing", "negative", "beyond"])
def test_refused_offsets(pkg, on_device, bad):
    """The rows handed over are the middle third of a three times larger allocation, so that even the refused offsets
    point inside it: the test checks the refusal and could not provoke an access out of bounds."""
    from locations_recommender_amd import _lib as L
    n, nseg, limit = 100, 3, 4
    offsets = {"decreasing": [0, 60, 30, 100], "negative": [-1, 10, 20, 100], "beyond": [0, 10, 20, 101]}[bad]
    arrays = dict(off=np.array(offsets, np.int64), ids=np.arange(3 * n, dtype=np.int64), scores=np.ones(3 * n),
                  pl=np.arange(3 * n, dtype=np.int64), reg=np.zeros(3 * n, np.int64), tgt=np.zeros(nseg, np.int64),
                  oi=np.full(nseg * limit, 77, np.int64), osc=np.full(nseg * limit, 7.5), oc=np.full(nseg, 77, np.int64))
    if on_device:
        arrays = {k: dev(v) for k, v in arrays.items()}
        torch.cuda.synchronize()
        p = {k: v.data_ptr() for k, v in arrays.items()}
    else:
        p = {k: v.ctypes.data for k, v in arrays.items()}
    st = L.lib().locrec_rank_recommendations_batch(nseg, C.c_void_p(p["off"]), n, C.c_void_p(p["ids"] + 8 * n),
                                                   C.c_void_p(p["scores"] + 8 * n), 3 * n, C.c_void_p(p["pl"]),
                                                   C.c_void_p(p["reg"]), C.c_void_p(p["tgt"]), limit,
                                                   L.MEM_DEVICE if on_device else L.MEM_HOST, C.c_void_p(p["oi"]),
                                                   C.c_void_p(p["osc"]), C.c_void_p(p["oc"]))
    assert st == L.E_INVALID_ARG
    oi, osc, oc = host((arrays["oi"], arrays["osc"], arrays["oc"]))
    assert (oi == 77).all() and (osc == 7.5).all() and (oc == 77).all()          # nothing written
    with pytest.raises(pkg.IllegalArgumentException):
        L.check(st)
