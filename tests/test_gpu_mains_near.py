"""GPU: within reach through the mains' request loops (mains.knn_recommender_requests_near,
mains.sg_recommender_requests_near) on the small generated sets of test_gpu_mains_new_places.  Expected: every line's
own rows - without the line's list where new_places - ranked by the oracle against the place table cut by
prep.distance_meters(position, place) <= radius, with the distance of each row's first kept listing."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import rank_near_cases as rn
from test_gpu_mains_new_places import KNN_RTOL
from test_mains import knn_files

pytestmark = pytest.mark.gpu
PW, CW, K, LIMIT = 0.5, 0.5, 50, 10


@pytest.fixture
def mains(pkg):
    from locations_recommender_amd import mains
    return mains


def write_places(tmp_path, seed=6):
    """Places 40..339 in regions 0 and 2, with coordinates by rank_near_cases' scheme."""
    place_ids = np.arange(40, 340, dtype=np.int64)
    regions = np.where(place_ids % 2 == 0, 0, 2).astype(np.int64)
    lat, lon = rn.coordinates(seed, regions)
    pq.write_table(pa.table({"id": place_ids, "latitude": lat, "longitude": lon, "region_id": pa.array(regions, pa.int32()),
                             "category_id": pa.array(place_ids % 7, pa.int32())}), tmp_path / "places_sample")
    return place_ids, regions, lat, lon


def positions_for(lines_target, regions, lat, lon, seed=2):
    """Per line a position on a place of its target region (line 0: the box centre); lines without a target: (0, 0)."""
    rng = np.random.default_rng(seed)
    plat, plon = np.zeros(len(lines_target)), np.zeros(len(lines_target))
    for i, t in enumerate(lines_target):
        if t is None:
            continue
        j = rng.choice(np.flatnonzero(regions == t))
        plat[i], plon[i] = lat[j], lon[j]
    t0 = lines_target[0]
    plat[0], plon[0] = rn.CORNERS[t0][0] + rn.BOX / 2, float(rn.wrap(np.float64(rn.CORNERS[t0][1] + rn.BOX / 2)))
    return plat, plon


def want_line(pkg, oracle, triple, pi, ps, table, position, radius):
    """One line through the composition: the place table cut by the device haversine, the oracle's ranker, the distance of
    each row's first kept listing."""
    place_ids, regions, lat, lon = table
    rows = np.flatnonzero(regions == triple[2])
    d = pkg.prep.distance_meters(np.full(len(rows), position[0]), np.full(len(rows), position[1]), lat[rows], lon[rows])
    rows, d = rows[d <= radius], d[d <= radius]
    oi, osc = oracle.rank_recommendations(pi, ps, place_ids[rows], regions[rows], triple[2], LIMIT)
    om = np.array([d[np.flatnonzero(place_ids[rows] == i)[0]] for i in np.asarray(oi)], np.float64)
    return triple, np.asarray(oi), np.asarray(osc), om


def check_lines(got, lines_want, rtol=0.0):
    assert len(got) == len(lines_want)
    for g, w in zip(got, lines_want):
        if isinstance(w, type):
            assert isinstance(g, w), (g, w)
            continue
        assert g[0] == w[0] and g[1].tolist() == w[1].tolist(), (g, w)
        if rtol:
            np.testing.assert_allclose(g[2], w[2], rtol=rtol, atol=0)
        else:
            assert g[2].tobytes() == w[2].tobytes(), (g, w)
        assert g[3].tobytes() == w[3].tobytes(), (g, w)


def test_knn_near(mains, tmp_path, pkg, oracle):
    from locations_recommender_amd import synth
    d = synth.knn_dataset(1_500, 300, seed=9)
    knn_files(tmp_path, d)
    table = write_places(tmp_path)
    ids = d["person_ids"]
    stranger = int(ids.max()) + 1                                      # in persons_sample, in no index
    home = np.zeros(len(ids) + 1, np.int64)
    home[[77, 4]] = 2                                                  # every line's region set is {0, 2}
    persons = {"id": np.r_[ids, stranger].astype(np.int64), "home_region_id": home}
    rows = [3, 900, 3, 1499, 77, 4]
    lines = [f"{ids[3]} 2", f"{ids[900]} 2", f"{ids[3]} 2", f"{ids[1499]} 2", "no number", f"{ids[77]} 0", f"{stranger} 2",
             f"{ids[4]} 0"]
    at = {0: 0, 1: 1, 2: 2, 3: 3, 5: 4, 7: 5}                          # good line -> position in rows
    targets = {0: 2, 1: 2, 2: 2, 3: 2, 5: 0, 7: 0}
    pos = positions_for([targets.get(i) for i in range(len(lines))], table[1], table[2], table[3])
    radii = np.array([1500.0, 400.0, 400.0, np.inf, 5.0, 60.0, 5.0, 1e5])
    ix = mains.knn_index_from_parquet(str(tmp_path), [0, 2])
    off, rp, re = ix.recommend_batch(ids[rows], PW, CW, K)
    ix.close()
    rated = {r: d["p_idx"][d["p_rowptr"][r]:d["p_rowptr"][r + 1]].astype(np.int64) for r in rows}   # knn_files' place_ratings

    def want(new_places, radius):
        out = []
        for i in range(len(lines)):
            if i not in at:
                out.append(pkg.IllegalArgumentException)
                continue
            r = rows[at[i]]
            pi, ps = rp[off[at[i]]:off[at[i] + 1]], re[off[at[i]]:off[at[i] + 1]]
            keep = ~np.isin(pi, rated[r]) if new_places else np.ones(len(pi), bool)
            out.append(want_line(pkg, oracle, (int(ids[r]), int(home[r]), targets[i]), pi[keep], ps[keep], table,
                                 (pos[0][i], pos[1][i]), radius[i]))
        return out

    per_line = want(False, radii)
    counts = [len(w[1]) for w in per_line if not isinstance(w, type)]
    assert min(counts) < LIMIT and max(counts) == LIMIT                                          # the circles bite
    got = mains.knn_recommender_requests_near(str(tmp_path), persons, lines, pos, radii, PW, CW, K, LIMIT)
    check_lines(got, per_line, KNN_RTOL)
    scalar = np.full(len(lines), 800.0)
    check_lines(mains.knn_recommender_requests_near(str(tmp_path), persons, lines, pos, 800.0, PW, CW, K, LIMIT),
                want(False, scalar), KNN_RTOL)
    new = want(True, scalar)
    check_lines(mains.knn_recommender_requests_near(str(tmp_path), persons, lines, pos, 800.0, PW, CW, K, LIMIT, new_places=True),
                new, KNN_RTOL)
    for i in at:
        assert not np.isin(new[i][1], rated[rows[at[i]]]).any()
    pkg.lib().locrec_cache_clear()


def test_sg_near(mains, tmp_path, pkg, oracle):
    from locations_recommender_amd import synth
    g = synth.sg_dataset(n_persons=1_200, n_places=300, seed=8)
    pq.write_table(pa.table({"source_id": g["source_id"], "target_id": g["target_id"],
                             "balanced_weight": g["balanced_weight"]}), tmp_path / "stochastic_graph_region0_region2")
    table = write_places(tmp_path)
    v0 = int(g["first_person"])
    stranger = 10 ** 9                                                  # in persons_sample, in no graph
    pid = np.r_[v0 + np.arange(1_200), stranger].astype(np.int64)
    home = np.zeros(len(pid), np.int64)
    home[12] = 2                                                        # every line's region set is {0, 2}
    persons = {"id": pid, "home_region_id": home}
    lines = [f"{v0 + 3} 2", f"{v0 + 700} 2", f"{v0 + 3} 2", "x 1", f"{stranger} 2", f"{v0 + 11} 2", f"{v0 + 12} 0"]
    good = {0: (v0 + 3, 2), 1: (v0 + 700, 2), 2: (v0 + 3, 2), 5: (v0 + 11, 2), 6: (v0 + 12, 0)}
    pos = positions_for([good[i][1] if i in good else None for i in range(len(lines))], table[1], table[2], table[3])
    radii = np.array([1500.0, 400.0, 400.0, 5.0, 5.0, np.inf, 60.0])
    visited = {}
    for s, t in zip(g["source_id"].tolist(), g["target_id"].tolist()):
        visited.setdefault(s, set()).add(t)
    rows = {v: mains.sg_make_recommendations(str(tmp_path), [0, 2], v, 0.01, 20)[:2] for v, _ in good.values()}

    def want(new_places, radius):
        out = []
        for i in range(len(lines)):
            if i not in good:
                out.append(pkg.IllegalArgumentException)
                continue
            v, t = good[i]
            pi, ps = rows[v]
            keep = ~np.isin(pi, sorted(visited[v])) if new_places else np.ones(len(pi), bool)
            out.append(want_line(pkg, oracle, (v, int(home[v - v0]), t), pi[keep], ps[keep], table, (pos[0][i], pos[1][i]),
                                 radius[i]))
        return out

    per_line = want(False, radii)
    counts = [len(w[1]) for w in per_line if not isinstance(w, type)]
    assert min(counts) < LIMIT and max(counts) == LIMIT                                          # the circles bite
    check_lines(mains.sg_recommender_requests_near(str(tmp_path), persons, lines, pos, radii, 0.01, 20, LIMIT), per_line)
    scalar = np.full(len(lines), 800.0)
    check_lines(mains.sg_recommender_requests_near(str(tmp_path), persons, lines, pos, 800.0, 0.01, 20, LIMIT), want(False, scalar))
    new = want(True, scalar)
    check_lines(mains.sg_recommender_requests_near(str(tmp_path), persons, lines, pos, 800.0, 0.01, 20, LIMIT, new_places=True), new)
    for i, (v, _) in good.items():
        assert not np.isin(new[i][1], sorted(visited[v])).any()
    pkg.lib().locrec_cache_clear()
