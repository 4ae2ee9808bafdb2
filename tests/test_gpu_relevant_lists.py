"""prep.relevant_lists on host arrays and on device tensors against the dict model of tests/eval_limit_cases.py; the
chain holdout_split -> relevant_lists -> evaluate_ranked with every array on the device against the same chain on host
arrays and the models; and mains._evaluate_in_batches over batches of any size against one evaluation of the whole."""
import numpy as np
import pytest
import torch

import eval_cases as ec
import eval_limit_cases as lc

pytestmark = pytest.mark.gpu
HELD = ("person_id", "region_id", "place_id")
CUTOFFS = [1, 3, 10]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def assert_lists(got, want, on_device):
    for g, w in zip(got, want):
        assert torch.is_tensor(g) == on_device and (not on_device or g.is_cuda)
        assert host(g).dtype == np.int64 and np.array_equal(host(g), w)


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_lists_on_host_and_device(pkg, seed):
    held, persons, regions, _ = lc.lists_case(seed)
    want = lc.model_relevant_lists(held, persons, regions)
    assert want[0][-1] > len(persons) // 2
    for p, r in ((persons, regions), (persons.tolist(), regions.tolist()), (torch.as_tensor(persons), torch.as_tensor(regions))):
        assert_lists(pkg.prep.relevant_lists(held, p, r), want, False)
    on_device = {k: dev(v) for k, v in held.items()}
    for p, r in ((persons, regions), (persons.tolist(), regions.tolist()), (dev(persons), dev(regions))):
        assert_lists(pkg.prep.relevant_lists(on_device, p, r), want, True)


def test_no_triples_and_no_requests(pkg):
    held, persons, regions, _ = lc.lists_case(0)
    none = np.empty(0, np.int64)
    for move in (lambda a: a, dev):
        off, ids = pkg.prep.relevant_lists({k: move(none) for k in HELD}, move(persons), move(regions))
        assert host(off).tolist() == [0] * (len(persons) + 1) and len(ids) == 0 and torch.is_tensor(off) == torch.is_tensor(move(none))
        off, ids = pkg.prep.relevant_lists({k: move(v) for k, v in held.items()}, move(none), move(none))
        assert host(off).tolist() == [0] and len(ids) == 0 and torch.is_tensor(ids) == torch.is_tensor(move(none))


def requests_of(held):
    """one request per (person, region) of the sorted triples, where they lie"""
    hp, hr = held["person_id"], held["region_id"]
    if torch.is_tensor(hp):
        first = torch.ones(len(hp), dtype=torch.bool, device=hp.device)
    else:
        first = np.ones(len(hp), bool)
    first[1:] = (hp[1:] != hp[:-1]) | (hr[1:] != hr[:-1])
    return hp[first], hr[first]


def synthetic_rows(offsets, ids, width=10):
    """Row i: the first ids of list i at the even positions, strangers between them, and as many ids as i says."""
    n = len(offsets) - 1
    rec = 10 ** 9 + np.arange(n * width, dtype=np.int64).reshape(n, width)
    for i in range(n):
        mine = ids[offsets[i]:offsets[i + 1]][:width // 2]
        rec[i, :2 * len(mine):2] = mine
    return rec, (np.arange(n, dtype=np.int64) * 7) % (width + 1)


def test_split_lists_and_evaluation_stay_on_the_device(pkg):
    prep = pkg.prep
    visits, cut = lc.two_region_case()
    table = {k: dev(v) for k, v in visits.items()}
    results = []
    for t in (visits, table):
        on_device = t is table
        _, held = prep.holdout_split(t, cut, new_places_only=False)
        persons, regions = requests_of(held)
        off, ids = prep.relevant_lists(held, persons, regions)
        assert all(torch.is_tensor(a) == on_device for a in (held["place_id"], persons, off, ids))
        if not on_device:
            rec, counts = synthetic_rows(off, ids)
        got = prep.evaluate_ranked(dev(rec) if on_device else rec, dev(counts) if on_device else counts, off, ids, CUTOFFS,
                                   per_segment=True)
        assert all(torch.is_tensor(got[k]) == on_device for k in ("relevant", "hits", "metrics"))
        results.append((got, host(persons), host(regions), host(off), host(ids)))
    (a, *lists_a), (b, *lists_b) = results
    assert all(np.array_equal(x, y) for x, y in zip(lists_a, lists_b))
    assert a["evaluated"] == b["evaluated"]
    for k in ("means", "coverage", "relevant", "hits", "metrics"):
        x, y = np.ascontiguousarray(host(a[k])), np.ascontiguousarray(host(b[k]))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    # and both are the models' chain
    _, held = ec.model_holdout(visits["person_id"], visits["timestamp"], visits["place_id"], visits["region_id"], cut, False)
    cols = np.array(held, np.int64)
    held = dict(zip(HELD, cols.T))
    persons, regions = requests_of(held)
    off, ids = lc.model_relevant_lists(held, persons, regions)
    assert np.array_equal(off, lists_a[2]) and np.array_equal(ids, lists_a[3]) and len(persons) > 60
    want = ec.model_eval(rec, counts, off, ids, CUTOFFS)
    assert want["hits"].sum() > 0 and want["evaluated"] == len(persons) and (want["hits"][:, -1] == 0).any()
    ec.assert_matches_model({k: host(v) if k != "evaluated" else v for k, v in b.items()}, want, CUTOFFS, len(persons))


def test_batches_of_any_size_add_up(pkg):
    from locations_recommender_amd import mains
    visits, cut = lc.two_region_case()
    _, held = ec.model_holdout(visits["person_id"], visits["timestamp"], visits["place_id"], visits["region_id"], cut, True)
    held = dict(zip(HELD, np.ascontiguousarray(np.array(held, np.int64).T)))
    persons, regions = requests_of(held)
    n = len(persons)
    off, ids = lc.model_relevant_lists(held, persons, regions)
    rec, counts = synthetic_rows(off, ids)
    counts[3::7] = np.minimum(counts[3::7], 2)
    rec[np.arange(10)[None, :] >= counts[:, None]] = -1
    row_of = {(int(p), int(r)): i for i, (p, r) in enumerate(zip(persons, regions))}
    widths = []

    def rank(p, r, k):
        """the fixed rows of the requests asked for, as wide as the longest of them: often narrower than k"""
        assert k == max(CUTOFFS)
        rows = [row_of[(int(a), int(b))] for a, b in zip(p, r)]
        width = max(1, int(counts[rows].max()))
        widths.append(width)
        return rec[rows, :width].copy(), counts[rows].copy()

    want = ec.model_eval(rec, counts, off, ids, CUTOFFS)
    assert want["evaluated"] > 0 and want["hits"].sum() > 0
    for batch in (1, 7, n):
        del widths[:]
        got = mains._evaluate_in_batches(rank, held, persons, regions, CUTOFFS, batch)
        assert len(widths) == -(-n // batch) and (batch == n or min(widths) < max(CUTOFFS))
        assert got["evaluated"] == want["evaluated"]
        assert np.array_equal(got["relevant"], want["relevant"]) and np.array_equal(got["coverage"], want["coverage"])
        assert np.array_equal(got["person_ids"], persons) and np.array_equal(got["region_ids"], regions)
        for j, k in enumerate(CUTOFFS):
            tol = (n + 4 * (k + 2)) * ec.U
            assert (np.abs(got["means"][j] - want["means"][j]) <= tol * np.abs(want["means"][j])).all(), (batch, k)
