"""GPU: mains.knn_visitor_requests on a small generated data directory - the region set's index from the handle cache,
the visitors' vectors from their visits (prep.visitor_vectors), one ranked visitors call.  Expected: the index
prep.knn_index_from_visits builds over the same visits PLUS the visitor's, asked through recommend_ranked_batch(...,
unvisited=new_places) for the visitor's id - one such index per visitor, as the contract has it (P + {v}): ids and counts
equal, scores within 1e-6."""
import numpy as np
import pytest

from test_gpu_mains_ranked import write_places
from test_mains import knn_files

pytestmark = pytest.mark.gpu
PW, CW, LIMIT = 0.5, 0.5, 10


def visits_of(n_persons, first_id, n_places, seed):
    """(person, place, category) visit rows: 5 .. 40 visits a person over a few favourite places."""
    rng = np.random.default_rng(seed)
    per = rng.integers(5, 41, n_persons)
    person = np.repeat(np.arange(first_id, first_id + n_persons, dtype=np.int64), per)
    place = (40 + np.minimum(rng.zipf(1.3, len(person)) - 1, n_places - 1)).astype(np.int64)
    return person, place, place % 12


@pytest.mark.parametrize("k", (30, 2_000_000))
def test_visitor_requests_equal_the_index_built_with_the_visitors(pkg, tmp_path, k):
    from locations_recommender_amd import mains, prep
    n, nv, n_places = 800, 21, 300
    person, place, cat = visits_of(n, 1000, n_places, seed=3)
    vperson, vplace, vcat = visits_of(nv, 50_000, n_places + 60, seed=4)      # some places no person of the index knows
    # the data directory: the rating vectors of the persons alone, as rating_vectors_builder_main writes them
    pp, pe, pr = prep.calc_ratings(person, place, prep.VISITED_PLACES_TOP_N)
    cp, ce, cr = prep.calc_ratings(person, cat, prep.VISITED_CATEGORIES_TOP_N)
    ids, p_ptr, p_idx, p_val, p_dim = prep.calc_rating_vectors(pp, pe, pr)
    _, c_ptr, c_idx, c_val, c_dim = prep.calc_rating_vectors(cp, ce, cr)
    d = dict(person_ids=ids, p_rowptr=p_ptr, p_idx=p_idx, p_val=p_val, p_dim=p_dim, c_rowptr=c_ptr, c_idx=c_idx, c_val=c_val, c_dim=c_dim)
    knn_files(tmp_path, d)
    place_ids = np.arange(40, 40 + n_places + 60, dtype=np.int64)
    regions = np.where(place_ids % 2 == 0, 0, 2)
    write_places(tmp_path, place_ids, regions)
    visitors = np.arange(50_000, 50_000 + nv, dtype=np.int64)
    targets = np.where(visitors % 3 == 0, 0, 2)
    visits = {"visitor_id": vperson, "place_id": vplace, "category_id": vcat}
    # the parent's way: the index rebuilt around the visitor.  One index per visitor - in ONE index over everybody the
    # other visitors would be persons, candidates of this one with rating rows of their own, which the contract excludes
    want = {False: [], True: []}
    for vid, t in zip(visitors, targets):
        m = vperson == vid
        one = prep.knn_index_from_visits(np.r_[person, vperson[m]], np.r_[place, vplace[m]], np.r_[cat, vcat[m]])
        for new_places in (False, True):
            want[new_places].append(one.recommend_ranked_batch([vid], PW, CW, k, place_ids, regions, [t], LIMIT, unvisited=new_places))
        one.close()
    assert vplace.max() >= p_dim                                               # entries beyond the index's dimensions
    for new_places in (False, True):
        wi, ws, wc = (np.concatenate([w[j] for w in want[new_places]]) for j in range(3))
        got = mains.knn_visitor_requests(str(tmp_path), [0, 2], visits, targets, PW, CW, k, LIMIT, new_places=new_places)
        assert [g[0] for g in got] == visitors.tolist()
        assert sum(int(c) for c in wc) > nv
        for i, (vid, gi, gs) in enumerate(got):
            assert len(gi) == wc[i] and gi.tolist() == wi[i, :wc[i]].tolist(), (i, gi, wi[i])
            np.testing.assert_allclose(gs, ws[i, :wc[i]], rtol=1e-6, atol=0)
            if new_places:
                assert not np.isin(gi, vplace[vperson == vid]).any()
        st = pkg.KnnIndex.visitors_stats()
        assert st["tiles"] == 2 and st["beyond"] > 0 and (st["tiles_all"] == 2) == (k >= n)
    # a mapping of targets, and CUDA tensors for the visits: the same answer
    import torch
    dev = {key: torch.from_numpy(v).cuda() for key, v in visits.items()}
    again = mains.knn_visitor_requests(str(tmp_path), [0, 2], dev, dict(zip(visitors.tolist(), targets.tolist())), PW, CW, k, LIMIT,
                                       new_places=True)
    assert all(a[0] == b[0] and a[1].tolist() == b[1].tolist() and a[2].tobytes() == b[2].tobytes() for a, b in zip(again, got))
    pkg.lib().locrec_cache_clear()
