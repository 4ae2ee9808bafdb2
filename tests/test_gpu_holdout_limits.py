"""GPU checks of locrec_holdout_split (csrc/eval.hip) at its limits, on the cases of tests/eval_limit_cases.py: (person,
place) pairs that lie in several regions, ids and times at the ends of int64 with the cut at either end, tables of
which no row or one triple is kept, a table far beyond one block of the device's sorts and selections, and the C call on
device memory - count only, a capacity below the count, no train rows wanted.  The reference is the set model of
tests/eval_cases.py: exact equality of the train rows and of the sorted triples."""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_cases as ec
import eval_limit_cases as lc

pytestmark = pytest.mark.gpu
COLUMNS = ("person_id", "timestamp", "place_id", "region_id", "category_id")


def dev_table(t):
    return {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in t.items()}


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def model(visits, cut, new_only):
    return ec.model_holdout(visits["person_id"], visits["timestamp"], visits["place_id"], visits["region_id"], cut, new_only)


def check(prep, visits, cut, new_only, on=("host", "device")):
    train_rows, held = model(visits, cut, new_only)
    want = np.array(held, np.int64).reshape(-1, 3)
    for where in on:
        table = visits if where == "host" else dev_table(visits)
        train, got = prep.holdout_split(table, cut, new_places_only=new_only)
        assert torch.is_tensor(train["person_id"]) == torch.is_tensor(got["person_id"]) == (where == "device")
        for k in COLUMNS:
            assert np.array_equal(host(train[k]), visits[k][train_rows]), k
        for j, k in enumerate(("person_id", "region_id", "place_id")):
            assert host(got[k]).dtype == np.int64 and np.array_equal(host(got[k]), want[:, j]), k
    return len(train_rows), len(held)


@pytest.mark.parametrize("new_only", (False, True))
def test_pairs_in_several_regions(pkg, new_only):
    visits, cut = lc.two_region_case()
    nt, nh = check(pkg.prep, visits, cut, new_only)
    assert 0 < nt < 3000 and nh > 0


@pytest.mark.parametrize("new_only", (False, True))
def test_ids_times_and_cuts_at_the_ends_of_int64(pkg, new_only):
    visits, cuts = lc.extreme_ids_case()
    n = len(visits["person_id"])
    sizes = [check(pkg.prep, visits, cut, new_only) for cut in cuts]
    assert sizes[0] == (0, 0)                                 # the cut at MIN: nothing is train, nobody to hold
    assert all(0 < nt < n and nh > 0 for nt, nh in sizes[1:])
    assert sizes[3][0] == int((visits["timestamp"] != ec.I64_MAX).sum())


def test_train_rows_and_nothing_kept(pkg):
    for visits, cut, new_only, kept_otherwise in lc.nothing_kept_cases():
        nt, nh = check(pkg.prep, visits, cut, new_only)
        assert nt > 0 and nh == 0
        assert (check(pkg.prep, visits, cut, not new_only)[1] > 0) == kept_otherwise


@pytest.mark.parametrize("new_only", (False, True))
def test_one_triple_many_times(pkg, new_only):
    visits, cut = lc.one_triple_case()
    assert check(pkg.prep, visits, cut, new_only) == (1, 1)


@pytest.mark.parametrize("new_only", (False, True))
def test_a_table_of_many_blocks(pkg, new_only):
    visits, cut = lc.multi_block_case()
    nt, nh = check(pkg.prep, visits, cut, new_only, on=("device",))
    assert 30_000 < nt < 40_000 and nh > 10_000


def test_the_c_call_on_device_memory(pkg):
    from locations_recommender_amd import _lib as L
    visits, cut = lc.two_region_case()
    n = len(visits["person_id"])
    train_rows, held = model(visits, cut, False)
    want = np.array(held, np.int64)
    assert len(held) > 10
    table = dev_table(visits)
    cols = [C.c_void_p(table[k].data_ptr()) for k in ("person_id", "timestamp", "place_id", "region_id")]
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(rows, outs, cap):
        nt, nh = np.full(1, -7, np.int64), np.full(1, cap, np.int64)
        torch.cuda.synchronize()
        st = L.lib().locrec_holdout_split(n, *cols, cut, 0, L.MEM_DEVICE, p(rows), L.ptr(nt, C.c_int64), *[p(o) for o in outs],
                                          L.ptr(nh, C.c_int64))
        assert st == L.OK, L.lib().locrec_last_error()
        torch.cuda.synchronize()
        return int(nt[0]), int(nh[0])

    sizes = (len(train_rows), len(held))
    assert call(None, (None, None, None), 0) == sizes                                      # count only
    rows = torch.full((n,), -7, dtype=torch.int32).cuda()
    outs = [torch.full((10,), -7, dtype=torch.int64).cuda() for _ in range(3)]
    assert call(rows, outs, 5) == sizes                                                    # the first five, the whole count
    assert rows[:len(train_rows)].tolist() == train_rows and bool((rows[len(train_rows):] == -7).all())
    for j, o in enumerate(outs):
        assert o[:5].tolist() == want[:5, j].tolist() and bool((o[5:] == -7).all())
    full = [torch.full((n,), -7, dtype=torch.int64).cuda() for _ in range(3)]
    assert call(None, full, n) == sizes                                                    # no train rows wanted
    for j, o in enumerate(full):
        assert o[:len(held)].tolist() == want[:, j].tolist() and bool((o[len(held):] == -7).all())
