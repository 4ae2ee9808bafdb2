"""The inputs of the pool-visitors tests (tests/knn_pool_visitor_cases.py) have the shapes their GPU tests rely on: block
counts, distinct place dimensions, finish tiles, segments, waves, staged lengths, who shares at each K.  No GPU."""
import numpy as np

import knn_pool_visitor_cases as pc


def test_members_have_the_shapes_that_select_the_shared_launches_paths():
    ds = pc.members()
    n = [len(d["person_ids"]) for d in ds]
    assert n == [200, 257, 3000, 4200, 200, 200, 0]
    blocks = [(x + 255) // 256 for x in n]
    assert blocks[:4] == [1, 2, 12, 17]                               # scan blocks: the grid is the largest member's
    assert len({d["p_dim"] for d in ds}) >= 4                         # bitmap sizes
    assert np.all(ds[0]["p_val"] == np.round(ds[0]["p_val"]))         # integer counts: such an index renumbers its places
    assert not np.all(ds[1]["p_val"] == np.round(ds[1]["p_val"]))     # the GENERIC format
    rated = [pc.rated_places(d) for d in ds]
    assert rated[2] > pc.FINISH_TILE and max(rated[0], rated[1], rated[3]) <= pc.FINISH_TILE   # two finish tiles; one
    assert rated[4] == 0 and rated[6] == 0
    assert np.bincount(ds[3]["r_place"]).max() > pc.SEG_RATERS        # more than 4,096 raters of one place: two segments
    assert np.bincount(ds[3]["r_place"])[7] == 4200
    assert np.bincount(ds[2]["r_place"]).max() <= pc.SEG_RATERS


def test_who_shares_at_each_k():
    n = [len(d["person_ids"]) for d in pc.members()]
    asked = sorted(pc.ASKED)
    assert [pc.way(2_000_000, n[m]) for m in asked] == ["shared"] * 5 + ["empty"]
    assert [pc.way(3_000, n[m]) for m in asked] == ["shared", "shared", "shared", "delegated", "shared", "empty"]
    assert [pc.way(50, n[m]) for m in asked] == ["delegated"] * 5 + ["empty"]
    assert pc.way(3000, 3000) == "shared" and pc.way(2999, 3000) == "delegated" and pc.way(1024, 200) == "delegated"


def test_visitors_are_interleaved_and_cut_into_three_waves():
    gi, vs, names = pc.visitors()
    ds = pc.members()
    assert len(gi) == len(vs) == sum(pc.ASKED.values()) == 45
    assert {int(m): int(np.sum(gi == m)) for m in np.unique(gi)} == pc.ASKED and 5 not in gi
    assert np.sum(np.diff(gi) != 0) >= 10                              # interleaved, not member after member
    waves = max(-(-c // pc.QT) for m, c in pc.ASKED.items() if m not in (4, 6))
    assert waves == 3 and pc.ASKED[2] % pc.QT == 5                     # the last tile partial
    at2 = np.flatnonzero(gi == 2)
    assert names["long"] == at2[0]                                     # in member 2's first tile: wave 0, beside the short tiles
    a, b = names["twice"]
    assert gi[a] == gi[b] == 2 and all(np.array_equal(vs[a][key], vs[b][key]) for key in vs[a])
    assert list(at2).index(a) // pc.QT != list(at2).index(b) // pc.QT  # ... in different tiles
    a, b = names["shared"]
    assert (gi[a], gi[b]) == (0, 1) and vs[a] is vs[b]
    assert 450 in vs[a]["p_idx"] and ds[0]["p_dim"] <= 450 < ds[1]["p_dim"]
    assert np.all(vs[a]["p_val"] == np.round(vs[a]["p_val"]))          # member 0 renumbers: integer counts
    for m, v in zip(gi, vs):                                           # what the stage accepts
        for fam in "pc":
            assert len(v[fam + "_idx"]) > 0 and np.all(np.diff(v[fam + "_idx"]) > 0) and v[fam + "_idx"][0] >= 0
            assert np.all(np.isfinite(v[fam + "_val"])) and np.any(v[fam + "_val"] != 0)
        if m != 1:
            assert np.all(v["p_val"] == np.round(v["p_val"])) and np.all(np.abs(v["p_val"]) < 65536)
    assert not np.all(vs[np.flatnonzero(gi == 1)[1]]["p_val"] == np.round(vs[np.flatnonzero(gi == 1)[1]]["p_val"]))


def test_staged_lengths_and_entries_beyond_the_dimensions():
    gi, vs, names = pc.visitors()
    ds = pc.members()
    lens = pc.staged_lengths()
    for i, (m, v) in enumerate(zip(gi, vs)):                           # every visitor has entries beyond the dimensions
        assert v["p_idx"][-1] >= ds[m]["p_dim"] and v["c_idx"][-1] >= ds[m]["c_dim"], i
        assert lens[1, i] > 0
    assert lens[0, names["long"]] == pc.LONG_ENTRIES > pc.FILL_BLOCK   # two fill blocks ...
    others = np.delete(np.arange(len(gi)), names["long"])
    assert lens[:, others].max() <= pc.FILL_BLOCK                      # ... where every other vector needs one
    assert lens[0, names["all_beyond"]] == 0 and len(vs[names["all_beyond"]]["p_idx"]) == 3
    assert lens[0, others].min() == 0 and np.sum(lens[0] == 0) == 1
    assert pc.beyond_entries() >= 3 * len(gi) - 1
    a, b = names["shared"]
    assert lens[0, b] == lens[0, a] + 1                                # the entry at 450


def test_tables_targets_and_lists():
    gi, vs, names = pc.visitors()
    places, regions = pc.places_table()
    assert len(places) == len(regions) and places.min() < 0 and places.max() >= 5000
    t = pc.targets(1)
    assert len(t) == len(gi) and 99 in t and t[names["twice"][0]] != t[names["twice"][1]]
    off, ids = pc.exclusion_lists()
    assert len(off) == len(gi) + 1 and off[0] == 0 and off[-1] == len(ids) and np.all(np.diff(off) >= 0)
    assert np.sum(np.diff(off) == 0) >= len(gi) // 3
    arrays = pc.arrays()
    assert len(arrays[0]) == len(gi) + 1 and arrays[0][-1] == len(arrays[1]) == len(arrays[2])
    at, sub = pc.of_member(2)
    assert len(at) == 37 and sub[0][-1] == sum(len(vs[i]["p_idx"]) for i in at)
