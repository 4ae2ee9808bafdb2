"""The cases of tests/eval_limit_cases.py hold what they are named for (no library, no GPU), under the models of
tests/eval_cases.py: a GPU test that passes on them has met the limit it is about."""
import numpy as np

import eval_cases as ec
import eval_limit_cases as lc

I64_MIN, I64_MAX = ec.I64_MIN, ec.I64_MAX


def split(visits, cut, new_only):
    return ec.model_holdout(visits["person_id"], visits["timestamp"], visits["place_id"], visits["region_id"], cut, new_only)


# ---- the evaluator -------------------------------------------------------------------------------------------------------

def test_late_first_hits_lie_behind_all_miss_tiles():
    case, sets, firsts = lc.late_first_hit()
    rec, counts, off, rel = case
    assert firsts[:-1] == [63, 64, 65, 127, 128, 191, 199] and all(len(c) <= 8 for c in sets)
    assert sorted(k for c in sets[:2] for k in c) == sorted(k for f in firsts[:-1] for k in (f, f + 1))
    assert sets[2] == [64, 128, 192, 200]
    for s, first in enumerate(firsts):
        wanted = set(rel[off[s]:off[s + 1]].tolist())
        at = [r for r in range(200) if int(rec[s, r]) in wanted]
        assert at[0] == first and (2 <= len(at) - 1 <= 3 or first + 3 >= 200)
        m = ec.model_eval(rec[s:s + 1], counts[s:s + 1], [0, len(wanted)], rel[off[s]:off[s + 1]], [first, first + 1])
        assert m["metrics"][0, 0, 2] == 0.0 and m["metrics"][0, 1, 2] == 1.0 / (first + 1)
        assert m["hits"][0].tolist() == [0, 1]
    only_tile_2 = [r for r in range(200) if int(rec[-1, r]) in set(rel[off[-2]:off[-1]].tolist())]
    assert only_tile_2 and all(128 <= r < 192 for r in only_tile_2)


def test_seam_cutoffs_differ_between_neighbours():
    case, sets = lc.seam_cutoffs()
    rec, counts, off, rel = case
    assert counts.tolist() == [200, 193, 192, 128, 65, 64, 63] and sets == [list(c) for c in lc.SEAM_CUTOFFS]
    for seam in (64, 128, 192):
        assert {seam - 2, seam - 1, seam, seam + 1} <= set(lc.SEAM_HITS)
    for cutoffs in sets:
        m = ec.model_eval(rec, counts, off, rel, cutoffs)
        order = np.argsort(cutoffs)
        for i, j in zip(order, order[1:]):
            if cutoffs[j] <= 200:
                # some segment tells the two cutoffs apart by its hits
                assert (m["hits"][:, i] != m["hits"][:, j]).any(), (cutoffs[i], cutoffs[j])
            else:
                # a row ends at 200: beyond it only the divisor of the precision tells them apart
                assert (m["metrics"][:, i, 0] != m["metrics"][:, j, 0]).any(), (cutoffs[i], cutoffs[j])
    # every row ends elsewhere among the hits: no two see the same number of them
    assert len(set(ec.model_eval(rec, counts, off, rel, [200])["hits"][:, 0].tolist())) == len(counts)


def test_huge_cutoffs_and_the_precision_restated():
    case, sets = lc.huge_cutoffs()
    assert sets[0] == [2 ** 31, 2 ** 40, 2 ** 53, 2 ** 62, 2 ** 63 - 1, 65, 64, 1] and sets[1] == [7] * 8
    assert max(sets[0]) == I64_MAX and case[0].shape == (5, 65)
    m = ec.model_eval(*case, sets[0])
    assert m["hits"].sum() > 0 and m["relevant"].max() <= 65          # so min(R, k) is R at every cutoff from 65 on
    # exact at and below 2^53, one ulp above it
    assert lc.precision_matches([3 / 2 ** 53], [3], 2 ** 53) and not lc.precision_matches([np.nextafter(3 / 2 ** 53, 1)], [3], 2 ** 53)
    q = 3 / I64_MAX
    assert lc.precision_matches([np.nextafter(q, 1)], [3], I64_MAX) and lc.precision_matches([3 / 2.0 ** 63], [3], I64_MAX)
    assert not lc.precision_matches([np.nextafter(np.nextafter(q, 1), 1)], [3], I64_MAX)
    assert lc.precision_matches([0.0, 0.5], [0, 1], 2) and not lc.precision_matches([0.0, 0.5], [0, 2], 2)


def test_duplicate_runs_cross_the_64_lane_steps():
    rec, counts, off, rel = lc.duplicate_runs()
    m = ec.model_eval(rec, counts, off, rel, [70, 4, 3])
    assert m["relevant"].tolist() == [1, 129, 71]
    assert np.diff(off).tolist() == [130, 258, 140] and len(set(rel[:130].tolist())) == 1
    assert m["hits"][0].tolist() == [1, 1, 0] and int(rec[0, 3]) == int(rel[0]) == int(rec[0, 10])
    assert m["hits"][1, 0] > 20 and m["hits"][2, 0] > 10
    last = np.sort(rel[off[2]:])
    assert last[69] == last[0] < last[70]                    # the run of 70 sorts first: it crosses the step at lane 64


def test_segment_counts_and_the_sparse_lists():
    assert lc.SEGMENT_COUNTS == (2, 3, 4, 5, 64, 128, 129, 256, 257, 1025) and lc.SEGMENT_CUTOFFS == [1, 5, 64, 70]
    for n in lc.SEGMENT_COUNTS:
        case = lc.segment_count_case(n)
        assert case[0].shape == (n, 70)
        if n <= 129:
            m = ec.model_eval(*case, lc.SEGMENT_CUTOFFS)
            assert m["evaluated"] > 0 and m["hits"].sum() > 0
    rec, counts, off, rel = lc.segment_count_case(1025, sparse=True)
    lengths = np.diff(off)
    assert [s for s in range(1025) if lengths[s]] == list(range(0, 1025, 97))
    m = ec.model_eval(rec, counts, off, rel, lc.SEGMENT_CUTOFFS)
    assert m["evaluated"] == 11 and m["hits"].sum() > 0


# ---- the lists -----------------------------------------------------------------------------------------------------------

def test_model_relevant_lists_by_hand():
    held = {"person_id": [1, 1, 1, 2, 5], "region_id": [0, 0, 3, 0, 3], "place_id": [9, 4, 7, 9, 1]}
    off, ids = lc.model_relevant_lists(held, [5, 1, 3, 1, 2, 1], [3, 0, 0, 3, 3, 0])
    assert off.tolist() == [0, 1, 3, 3, 4, 4, 6] and ids.tolist() == [1, 9, 4, 7, 9, 4]
    off, ids = lc.model_relevant_lists(held, [], [])
    assert off.tolist() == [0] and ids.dtype == np.int64 and len(ids) == 0


def test_lists_case_has_every_kind_of_request():
    for seed in range(3):
        held, persons, regions, kinds = lc.lists_case(seed)
        triples = list(zip(*(held[k].tolist() for k in ("person_id", "region_id", "place_id"))))
        assert triples == sorted(set(triples)) and {I64_MIN, I64_MAX} <= set(held["region_id"].tolist()) | set(held["place_id"].tolist())
        off, ids = lc.model_relevant_lists(held, persons, regions)
        lengths = np.diff(off)
        assert set(kinds) == set(lc.LIST_KINDS) and lengths.max() > 3
        known_p, known_r = set(held["person_id"].tolist()), set(held["region_id"].tolist())
        for kind in lc.LIST_KINDS[1:]:
            assert all(lengths[i] == 0 for i, k in enumerate(kinds) if k == kind), kind
        at = lambda kind: [i for i, k in enumerate(kinds) if k == kind]
        assert all(lengths[i] > 0 for i in at("known"))
        pairs = list(zip(persons[at("known")].tolist(), regions[at("known")].tolist()))
        assert set(pairs) == {(p, r) for p, r, _ in triples} and len(pairs) > len(set(pairs))
        assert all(persons[i] < min(known_p) for i in at("below")) and all(persons[i] > max(known_p) for i in at("above"))
        for i in at("between") + at("unknown_person"):
            assert min(known_p) < persons[i] < max(known_p) and persons[i] not in known_p and regions[i] in known_r
        assert all(persons[i] in known_p and regions[i] not in known_r for i in at("unknown_region"))
        assert all(persons[i] in known_p and regions[i] in known_r for i in at("absent_pair"))


# ---- the split -----------------------------------------------------------------------------------------------------------

def test_two_region_case_has_pairs_in_several_regions():
    for maker, pairs_wanted in ((lc.two_region_case, 50), (lc.multi_block_case, 50)):
        v, cut = maker()
        train, held = split(v, cut, False)
        _, new = split(v, cut, True)
        regions_of = {}
        for p, r, place in held:
            regions_of.setdefault((p, place), set()).add(r)
        assert sum(1 for rs in regions_of.values() if len(rs) >= 2) >= pairs_wanted
        assert any(len(rs) == 3 for rs in regions_of.values())
        been = {(int(v["person_id"][i]), int(v["region_id"][i]), int(v["place_id"][i])) for i in train}
        other_region_only = [t for t in set(held) - set(new) if t not in been]
        assert len(other_region_only) >= 20                 # dropped for a train visit at the place under another region
        assert 0 < len(train) < len(v["person_id"]) and 0 < len(new) < len(held)
        assert v["person_id"].min() not in {p for p, _, _ in held}
    assert len(lc.two_region_case()[0]["person_id"]) == 3000 and len(lc.multi_block_case()[0]["person_id"]) == 70_000
    v = lc.multi_block_case()[0]
    assert len(set(v["person_id"].tolist())) == 2000 and len(set(v["place_id"].tolist())) == 500


def test_extreme_ids_case():
    v, cuts = lc.extreme_ids_case()
    ends = {I64_MIN, I64_MIN + 1, -1, 0, I64_MAX - 1, I64_MAX}
    assert cuts == (I64_MIN, I64_MIN + 1, 0, I64_MAX) and 30 <= len(v["person_id"]) <= 50
    for k in ("person_id", "place_id", "region_id"):
        assert set(v[k].tolist()) == ends, k
    assert set(v["timestamp"].tolist()) == ends | {1}
    assert split(v, I64_MIN, False) == ([], []) and split(v, I64_MIN, True) == ([], [])
    for cut in (I64_MIN + 1, 0):
        for new_only in (False, True):
            train, held = split(v, cut, new_only)
            assert train and held, (cut, new_only)
    train, held = split(v, I64_MAX, False)
    assert len(train) == int((v["timestamp"] != I64_MAX).sum()) and 0 < len(held) <= int((v["timestamp"] == I64_MAX).sum())
    assert len(split(v, I64_MAX, True)[1]) < len(held)
    # unseen persons between seen ones at the cut MIN + 1
    seen = set(v["person_id"][v["timestamp"] < I64_MIN + 1].tolist())
    assert seen == {I64_MIN, I64_MIN + 1, 0, I64_MAX}
    # the neighbour's table entry: a new place above all the person's train places that is the next person's smallest
    train, held = split(v, 0, True)
    places = {}
    for i in train:
        places.setdefault(int(v["person_id"][i]), set()).add(int(v["place_id"][i]))
    trapped = [(p, place) for p, _, place in held if p + 1 in places and place > max(places[p]) and place == min(places[p + 1])]
    assert {p for p, _ in trapped} == {I64_MIN, -1, I64_MAX - 1}
    # adjacent persons share places on both sides of the cut
    assert places[I64_MIN + 1] & places[0] and places[-1] & places[I64_MIN]


def test_the_exits_of_the_split():
    cases = lc.nothing_kept_cases()
    assert len(cases) == 3
    for v, cut, new_only, kept_otherwise in cases:
        train, held = split(v, cut, new_only)
        assert train and not held and (v["timestamp"] >= cut).any()
        assert bool(split(v, cut, not new_only)[1]) == kept_otherwise
    a = cases[0][0]
    train_persons = set(a["person_id"][a["timestamp"] < cases[0][1]].tolist())
    held_persons = set(a["person_id"][a["timestamp"] >= cases[0][1]].tolist())
    assert not train_persons & held_persons and min(held_persons) < min(train_persons) < max(train_persons) < max(held_persons)
    assert any(min(train_persons) < p < max(train_persons) for p in held_persons)
    v, cut = lc.one_triple_case()
    for new_only in (False, True):
        train, held = split(v, cut, new_only)
        assert len(train) == 1 and held == [(-12345, 2, 77)] and int((v["timestamp"] >= cut).sum()) == 500
