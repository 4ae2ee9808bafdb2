"""GPU: by category through the mains' request loops (mains.knn_recommender_requests_by_category,
mains.sg_recommender_requests_by_category) on the generated places_sample of test_gpu_mains_near, end to end against the
numpy restatement mains.rank_recommendations_by_category applied to every line's own rows."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from test_gpu_mains_near import positions_for, write_places
from test_gpu_mains_new_places import KNN_RTOL
from test_mains import knn_files

pytestmark = pytest.mark.gpu
PW, CW, K, LIMIT = 0.5, 0.5, 50, 10


@pytest.fixture
def mains(pkg):
    from locations_recommender_amd import mains
    return mains


def want_line(mains, pkg, triple, pi, ps, table, categories, cap, position=None, radius=None):
    """One line through the numpy restatement (its circle through the device haversine)."""
    place_ids, regions, lat, lon = table
    cats = place_ids % 7                                                   # write_places' category_id column
    allowed = None if categories is None else (np.array([0, len(categories)], np.int64), np.asarray(categories, np.int64))
    circles = None if position is None else (lat, lon, [position[0]], [position[1]], [radius])
    oi, osc, om, cnt = mains.rank_recommendations_by_category([0, len(pi)], pi, ps, place_ids, regions, [triple[2]], LIMIT, cats,
                                                              allowed=allowed, max_per_category=None if cap is None else [cap],
                                                              circles=circles)
    return triple, oi[0, :cnt[0]], osc[0, :cnt[0]], None if om is None else om[0, :cnt[0]]


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
        assert (g[3] is None and w[3] is None) or g[3].tobytes() == w[3].tobytes(), (g, w)


def test_knn_by_category(mains, tmp_path, pkg):
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
    ix = mains.knn_index_from_parquet(str(tmp_path), [0, 2])
    off, rp, re = ix.recommend_batch(ids[rows], PW, CW, K)
    ix.close()
    rated = {r: d["p_idx"][d["p_rowptr"][r]:d["p_rowptr"][r + 1]].astype(np.int64) for r in rows}   # knn_files' place_ratings

    def want(categories, caps, new_places=False, radius=None):
        out = []
        for i in range(len(lines)):
            if i not in at:
                out.append(pkg.IllegalArgumentException)
                continue
            r = rows[at[i]]
            pi, ps = rp[off[at[i]]:off[at[i] + 1]], re[off[at[i]]:off[at[i] + 1]]
            keep = ~np.isin(pi, rated[r]) if new_places else np.ones(len(pi), bool)
            cat = categories[i] if categories is not None and np.ndim(categories[0]) == 1 else categories
            cap = None if caps is None else (caps if np.ndim(caps) == 0 else caps[i])
            out.append(want_line(mains, pkg, (int(ids[r]), int(home[r]), targets[i]), pi[keep], ps[keep], table, cat, cap,
                                 None if radius is None else (pos[0][i], pos[1][i]), radius))
        return out

    free = want(None, None)
    capped = want(None, 2)
    assert any(f[1].tolist() != c[1].tolist() for f, c in zip(free, capped) if not isinstance(f, type))     # the cap bites
    check_lines(mains.knn_recommender_requests_by_category(str(tmp_path), persons, lines, PW, CW, K, LIMIT, max_per_category=2),
                capped, KNN_RTOL)
    only = want([1, 3], None)
    assert all(set((w[1] % 7).tolist()) <= {1, 3} for w in only if not isinstance(w, type))
    check_lines(mains.knn_recommender_requests_by_category(str(tmp_path), persons, lines, PW, CW, K, LIMIT, categories=[1, 3]),
                only, KNN_RTOL)
    per_line = [np.array([i % 7, (i + 2) % 7], np.int64) if i % 3 else np.empty(0, np.int64) for i in range(len(lines))]
    caps = np.arange(len(lines)) % 3 + 1
    check_lines(mains.knn_recommender_requests_by_category(str(tmp_path), persons, lines, PW, CW, K, LIMIT, categories=per_line,
                                                           max_per_category=caps, new_places=True, positions=pos,
                                                           radius_meters=1500.0),
                want(per_line, caps, True, 1500.0), KNN_RTOL)
    pkg.lib().locrec_cache_clear()


def test_sg_by_category(mains, tmp_path, pkg):
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
    visited = {}
    for s, t in zip(g["source_id"].tolist(), g["target_id"].tolist()):
        visited.setdefault(s, set()).add(t)
    rows = {v: mains.sg_make_recommendations(str(tmp_path), [0, 2], v, 0.01, 20)[:2] for v, _ in good.values()}

    def want(categories, caps, new_places=False, radius=None):
        out = []
        for i in range(len(lines)):
            if i not in good:
                out.append(pkg.IllegalArgumentException)
                continue
            v, t = good[i]
            pi, ps = rows[v]
            keep = ~np.isin(pi, sorted(visited[v])) if new_places else np.ones(len(pi), bool)
            cat = categories[i] if categories is not None and np.ndim(categories[0]) == 1 else categories
            cap = None if caps is None else (caps if np.ndim(caps) == 0 else caps[i])
            out.append(want_line(mains, pkg, (v, int(home[v - v0]), t), pi[keep], ps[keep], table, cat, cap,
                                 None if radius is None else (pos[0][i], pos[1][i]), radius))
        return out

    free, capped = want(None, None), want(None, 1)
    assert any(f[1].tolist() != c[1].tolist() for f, c in zip(free, capped) if not isinstance(f, type))     # the cap bites
    assert all(len(set((c[1] % 7).tolist())) == len(c[1]) for c in capped if not isinstance(c, type))
    check_lines(mains.sg_recommender_requests_by_category(str(tmp_path), persons, lines, 0.01, 20, LIMIT, max_per_category=1), capped)
    per_line = [np.array([i % 7, (i + 2) % 7, (i + 4) % 7], np.int64) if i % 3 else np.empty(0, np.int64) for i in range(len(lines))]
    caps = np.arange(len(lines)) % 3 + 1
    check_lines(mains.sg_recommender_requests_by_category(str(tmp_path), persons, lines, 0.01, 20, LIMIT, categories=per_line,
                                                          max_per_category=caps, new_places=True, positions=pos,
                                                          radius_meters=1500.0),
                want(per_line, caps, True, 1500.0))
    pkg.lib().locrec_cache_clear()
