"""GPU checks of locrec_holdout_split (csrc/eval.hip) through prep.holdout_split and the C call, against the set model of
tests/eval_cases.py: exact equality of the train rows and of the sorted held-out triples."""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_cases as ec

pytestmark = pytest.mark.gpu
COLUMNS = ("person_id", "timestamp", "place_id", "region_id", "category_id")


def dev_table(t):
    return {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in t.items()}


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def check(prep, visits, cut, new_only):
    train_rows, held = ec.model_holdout(visits["person_id"], visits["timestamp"], visits["place_id"], visits["region_id"], cut, new_only)
    want = np.array(held, np.int64).reshape(-1, 3)
    for table in (visits, dev_table(visits)):
        train, got = prep.holdout_split(table, cut, new_places_only=new_only)
        assert torch.is_tensor(train["person_id"]) == torch.is_tensor(table["person_id"])
        for k in COLUMNS:
            assert np.array_equal(host(train[k]), visits[k][train_rows]), k
        for j, k in enumerate(("person_id", "region_id", "place_id")):
            assert host(got[k]).dtype == np.int64 and np.array_equal(host(got[k]), want[:, j]), k
    return len(train_rows), len(held)


@pytest.mark.parametrize("new_only", (False, True))
def test_against_the_model(pkg, new_only):
    visits = ec.holdout_case(3, 2000)
    nt, nh = check(pkg.prep, visits, 1000, new_only)
    assert 0 < nt < 2000 and nh > 0
    one = {k: v[:1] for k, v in visits.items()}
    assert check(pkg.prep, one, int(one["timestamp"][0]), new_only) == (0, 0)          # equal to the cut: held out, nobody to hold
    assert check(pkg.prep, one, int(one["timestamp"][0]) + 1, new_only) == (1, 0)
    assert check(pkg.prep, {k: v[:0] for k, v in visits.items()}, 1000, new_only) == (0, 0)


def test_every_row_on_one_side(pkg):
    before = ec.holdout_case(5, 700, after=False)
    assert check(pkg.prep, before, 1000, True) == (700, 0)
    after = ec.holdout_case(6, 700, before=False)
    assert check(pkg.prep, after, 1000, False) == (0, 0)


def test_a_visited_place_is_kept_or_dropped_by_the_flag(pkg):
    visits = ec.holdout_case(3, 2000)
    _, every = pkg.prep.holdout_split(visits, 1000, new_places_only=False)
    _, new = pkg.prep.holdout_split(visits, 1000, new_places_only=True)
    every = set(zip(*(every[k].tolist() for k in ("person_id", "region_id", "place_id"))))
    new = set(zip(*(new[k].tolist() for k in ("person_id", "region_id", "place_id"))))
    been = set(zip(visits["person_id"][visits["timestamp"] < 1000].tolist(), visits["place_id"][visits["timestamp"] < 1000].tolist()))
    assert new < every and all((p, pl) in been for p, _, pl in every - new) and not any((p, pl) in been for p, _, pl in new)
    assert visits["person_id"].min() not in {p for p, _, _ in every}                       # seen only behind the cut: dropped


def test_count_only_and_a_capacity_too_small(pkg):
    from locations_recommender_amd import _lib as L
    visits = ec.holdout_case(3, 2000)
    train_rows, held = ec.model_holdout(visits["person_id"], visits["timestamp"], visits["place_id"], visits["region_id"], 1000, False)
    want = np.array(held, np.int64)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    cols = [np.ascontiguousarray(visits[k]) for k in ("person_id", "timestamp", "place_id", "region_id")]

    def call(rows, outs, cap):
        nt, nh = np.full(1, -7, np.int64), np.full(1, cap, np.int64)
        st = L.lib().locrec_holdout_split(2000, *[p(c) for c in cols], 1000, 0, L.MEM_HOST, p(rows), L.ptr(nt, C.c_int64),
                                          *[p(o) for o in outs], L.ptr(nh, C.c_int64))
        assert st == L.OK
        return int(nt[0]), int(nh[0])

    assert call(None, (None, None, None), 0) == (len(train_rows), len(held))               # count only
    rows = np.full(2000, -7, np.int32)
    outs = [np.full(10, -7, np.int64) for _ in range(3)]
    assert call(rows, [o[:5] for o in outs], 5) == (len(train_rows), len(held))            # the first five, and the whole count
    assert rows[:len(train_rows)].tolist() == train_rows and (rows[len(train_rows):] == -7).all()
    for j, o in zip((0, 1, 2), outs):
        assert o[:5].tolist() == want[:5, j].tolist() and (o[5:] == -7).all()
