"""GPU: mains.knn_visitor_requests_pooled on a small generated data directory with three region sets - every visitor's
index from the handle cache by [home, target], the vectors of all visitors from ONE prep.visitor_vectors call, one pool call.
Expected: the same call with pooled=False (one visitors call per distinct index) bit for bit, and, for the visitors of each
region set, mains.knn_visitor_requests on that region set alone."""
import numpy as np
import pytest

from test_gpu_mains_ranked import write_places
from test_gpu_mains_visitors import visits_of
from test_mains import knn_files

pytestmark = pytest.mark.gpu
PW, CW, LIMIT = 0.5, 0.5, 10
SETS = {(0, 0): "region0", (0, 2): "region0_region2", (1, 2): "region1_region2"}   # sorted{home, target} -> the files' suffix


def region_set_files(tmp_path, prep, name, n, first_id, n_places, seed):
    """The rating vectors of n persons' visits, as rating_vectors_builder_main writes them for one region set."""
    person, place, cat = visits_of(n, first_id, n_places, seed)
    pp, pe, pr = prep.calc_ratings(person, place, prep.VISITED_PLACES_TOP_N)
    cp, ce, cr = prep.calc_ratings(person, cat, prep.VISITED_CATEGORIES_TOP_N)
    ids, p_ptr, p_idx, p_val, p_dim = prep.calc_rating_vectors(pp, pe, pr)
    _, c_ptr, c_idx, c_val, c_dim = prep.calc_rating_vectors(cp, ce, cr)
    d = dict(person_ids=ids, p_rowptr=p_ptr, p_idx=p_idx, p_val=p_val, p_dim=p_dim, c_rowptr=c_ptr, c_idx=c_idx, c_val=c_val, c_dim=c_dim)
    knn_files(tmp_path, d, regions=name)
    return d


def same(a, b):
    return a[0] == b[0] and a[1].tolist() == b[1].tolist() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("k", (30, 2_000_000))
def test_pooled_visitor_requests(pkg, tmp_path, k):
    from locations_recommender_amd import mains, prep
    n_places = 300
    sizes = {"region0": (700, 1000, 280, 3), "region0_region2": (800, 5000, 300, 4), "region1_region2": (150, 9000, 200, 5)}
    ds = {name: region_set_files(tmp_path, prep, name, *args) for name, args in sizes.items()}
    assert len({d["p_dim"] for d in ds.values()}) == 3
    place_ids = np.arange(40, 40 + n_places + 60, dtype=np.int64)
    write_places(tmp_path, place_ids, place_ids % 3)
    nv = 40
    vperson, vplace, vcat = visits_of(nv, 50_000, n_places + 60, seed=6)      # some places no person of any index knows
    visitors = np.arange(50_000, 50_000 + nv, dtype=np.int64)
    pairs = [(0, 0), (0, 2), (2, 0), (1, 2), (2, 1)]
    homes = np.array([pairs[i % 5][0] for i in range(nv)], np.int64)
    targets = np.array([pairs[i % 5][1] for i in range(nv)], np.int64)
    homes[7], targets[7] = 5, 7                                               # a region set without files
    visits = {"visitor_id": vperson, "place_id": vplace, "category_id": vcat}
    assert vplace.max() >= max(d["p_dim"] for d in ds.values())               # entries beyond every index's dimensions
    got = {}
    for new_places in (False, True):
        for pooled in (True, False):
            got[new_places, pooled] = mains.knn_visitor_requests_pooled(str(tmp_path), visits, homes, targets, PW, CW, k, LIMIT,
                                                                        new_places=new_places, pooled=pooled)
            if pooled:
                st = pkg.KnnPool.visitors_stats()
                assert st["stage_launches"] == 1 and st["beyond"] > 0
                # 800 persons at most: every index shares at the shipped K, and 8, 15 and 16 visitors make one wave of three tiles
                assert (st["waves"], st["member_tiles"], st["delegated_members"]) == ((1, 3, 0) if k > 1024 else (0, 0, 3))
        a, b = got[new_places, True], got[new_places, False]
        assert len(a) == len(b) == nv
        for i in range(nv):
            if i == 7:                                                        # the exception instance; the others their answers
                assert isinstance(a[i], Exception) and isinstance(b[i], Exception) and type(a[i]) is type(b[i])
                continue
            assert a[i][0] == visitors[i] and same(a[i], b[i]), (new_places, i)
        assert sum(len(x[1]) for i, x in enumerate(a) if i != 7) > nv
        # the visitors of each region set through knn_visitor_requests on that region set alone
        for key, name in SETS.items():
            mine = np.flatnonzero([tuple(sorted((int(h), int(t)))) == tuple(sorted(key)) for h, t in zip(homes, targets)])
            assert len(mine) >= 7
            rows = np.isin(vperson, visitors[mine])
            sub = {"visitor_id": vperson[rows], "place_id": vplace[rows], "category_id": vcat[rows]}
            want = mains.knn_visitor_requests(str(tmp_path), list(key), sub, targets[mine], PW, CW, k, LIMIT, new_places=new_places)
            assert len(want) == len(mine)
            for w, i in zip(want, mine):
                assert same(a[i], w), (new_places, name, i)
                if new_places:
                    assert not np.isin(a[i][1], vplace[vperson == visitors[i]]).any()
    assert any(not same(x, y) for i, (x, y) in enumerate(zip(got[False, True], got[True, True])) if i != 7)
    # mappings for the regions and CUDA tensors for the visits: the same answer
    import torch
    dev = {key: torch.from_numpy(v).cuda() for key, v in visits.items()}
    again = mains.knn_visitor_requests_pooled(str(tmp_path), dev, dict(zip(visitors.tolist(), homes.tolist())),
                                              dict(zip(visitors.tolist(), targets.tolist())), PW, CW, k, LIMIT, new_places=True)
    assert all(isinstance(x, Exception) if i == 7 else same(x, y) for i, (x, y) in enumerate(zip(again, got[True, True])))
    pkg.lib().locrec_cache_clear()
