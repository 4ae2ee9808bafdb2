"""GPU checks of locrec_eval_ranked_batch (csrc/eval.hip) through prep.evaluate_ranked, against the set-and-fsum model of
tests/eval_cases.py: the widths around the 64-wide walk, one to 300 segments, the counts and lists of eval_case, host and
device inputs, and the tolerances of eval_cases.assert_matches_model (derived from the arithmetic, not measured)."""
import ctypes as C

import numpy as np
import pytest
import torch

import eval_cases as ec

pytestmark = pytest.mark.gpu
WIDTHS = (1, 63, 64, 65, 128, 129)
SEGMENTS = (1, 65, 300)
OUTPUTS = ("means", "coverage", "relevant", "hits", "metrics")


def cutoff_sets(width):
    return [[1], [width], [width + 7], [10, 1, 10, 5], [1, 2, 3, 5, 8, width, width + 1, 2 * width + 3]]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def same_bits(a, b):
    a, b = np.ascontiguousarray(host(a)), np.ascontiguousarray(host(b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same_outputs(a, b, names=OUTPUTS):
    assert a["evaluated"] == b["evaluated"]
    for k in names:
        assert same_bits(a[k], b[k]), k


def check_case(prep, case, cutoffs, repeat=False):
    rec, counts, off, rel = case
    want = ec.model_eval(rec, counts, off, rel, cutoffs)
    assert want["evaluated"] > 0 and want["hits"].sum() > 0, "a vacuous case"
    got = prep.evaluate_ranked(rec, counts, off, rel, cutoffs, per_segment=True)
    st = prep.evaluate_ranked_stats()
    assert st["path"] == 1 and st["evaluated"] == want["evaluated"] and st["table_entries"] == int(want["relevant"].sum())
    ec.assert_matches_model(got, want, cutoffs, len(counts))
    on_device = prep.evaluate_ranked(dev(rec), dev(counts), dev(off), dev(rel), cutoffs, per_segment=True)
    assert all(torch.is_tensor(on_device[k]) for k in ("relevant", "hits", "metrics"))
    assert_same_outputs(got, on_device)                     # host and device inputs: identical bits
    if repeat:
        assert_same_outputs(got, prep.evaluate_ranked(rec, counts, off, rel, cutoffs, per_segment=True))
        lean = prep.evaluate_ranked(rec, counts, off, rel, cutoffs)
        assert "hits" not in lean and "metrics" not in lean
        assert_same_outputs(got, lean, ("means", "coverage", "relevant"))
    return st


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n_segments", SEGMENTS)
def test_against_the_model(pkg, n_segments, width):
    case = ec.eval_case(n_segments * 1000 + width, n_segments, width)
    sets = cutoff_sets(width)
    for cutoffs in sets:
        check_case(pkg.prep, case, cutoffs, repeat=cutoffs is sets[-1])


def test_corner_case(pkg):
    """One id relevant in two segments and recommended in one, a repeated relevant id, -1 in a list beside a padded row,
    the extreme ids, an empty list, and offsets that start above 0."""
    for cutoffs in ([1, 4], [2], [4, 3, 2, 1, 9]):
        check_case(pkg.prep, ec.corner_case(), cutoffs, repeat=True)
    got = pkg.prep.evaluate_ranked(*ec.corner_case(), [4], per_segment=True)
    assert got["hits"][:, 0].tolist() == [1, 1, 2, 1, 3, 0] and got["relevant"].tolist() == [2, 1, 2, 2, 4, 0]
    assert got["evaluated"] == 5 and got["means"][0, 5] == 1.0


def test_rows_and_lists_beyond_any_lds_buffer(pkg):
    case = ec.wide_case()
    want = ec.model_eval(*case, [3000])
    first_list = set(case[3][:5000].tolist())
    beyond = [r for r in range(2048, 3000) if int(case[0][0, r]) in first_list]
    assert len(beyond) > 300, "hits beyond position 2048"
    check_case(pkg.prep, case, [3000, 2049, 10, 3007], repeat=True)
    assert want["hits"][0, 0] == pkg.prep.evaluate_ranked(*case, [3000], per_segment=True)["hits"][0, 0]


def test_host_synchronisations_do_not_depend_on_the_segments(pkg):
    syncs = []
    for n_segments in (1, 300):
        case = ec.eval_case(7 + n_segments, n_segments, 65)
        syncs.append(check_case(pkg.prep, case, [5, 65])["host_syncs"])
        pkg.prep.evaluate_ranked(*case, [5, 65])
        assert pkg.prep.evaluate_ranked_stats()["host_syncs"] == syncs[-1]
    assert syncs[0] == syncs[1] == 2


def test_empty_shapes(pkg):
    prep = pkg.prep
    none = np.empty(0, np.int64)
    got = prep.evaluate_ranked(np.empty((0, 5), np.int64), none, np.zeros(1, np.int64), none, [3, 1], per_segment=True)
    assert got["evaluated"] == 0 and not got["means"].any() and not got["coverage"].any() and got["hits"].shape == (0, 2)
    # width 0: nothing to read, the lists are still counted
    for move in (lambda a: a, dev):
        got = prep.evaluate_ranked(move(np.empty((3, 0), np.int64)), move(np.zeros(3, np.int64)), move(np.array([0, 2, 2, 3])),
                                   move(np.array([5, 5, 6])), [3], per_segment=True)
        assert host(got["relevant"]).tolist() == [1, 0, 1] and got["evaluated"] == 2
        assert not got["means"].any() and not got["coverage"].any() and not host(got["hits"]).any() and not host(got["metrics"]).any()


def test_refusals_on_device_arrays(pkg):
    """A bad rec_counts entry and decreasing rel_offsets are found on the device, before anything is read through them,
    and nothing is written."""
    from locations_recommender_amd import _lib as L
    rec, counts, off, rel = ec.eval_case(5, 65, 64)
    cut = np.array([3, 64], np.int64)

    def call(counts, off):
        d = [dev(rec.reshape(-1)), dev(counts), dev(off), dev(rel)]
        outs = [torch.full((65,), 77, dtype=torch.int64).cuda(), torch.full((130,), 77, dtype=torch.int64).cuda(),
                torch.full((650,), 7.5, dtype=torch.float64).cuda()]
        means, cov, ev = np.full(12, 7.5), np.full(2, 77, np.int64), np.full(1, 77, np.int64)
        torch.cuda.synchronize()
        st = L.lib().locrec_eval_ranked_batch(65, 64, *[C.c_void_p(t.data_ptr()) for t in d[:3]], len(rel), C.c_void_p(d[3].data_ptr()),
                                              2, L.ptr(cut, C.c_int64), L.MEM_DEVICE, *[C.c_void_p(t.data_ptr()) for t in outs],
                                              L.ptr(means, C.c_double), L.ptr(cov, C.c_int64), L.ptr(ev, C.c_int64))
        untouched = (all(bool((t == 77).all()) for t in outs[:2]) and bool((outs[2] == 7.5).all()) and (means == 7.5).all()
                     and (cov == 77).all() and ev[0] == 77)
        return st, L.lib().locrec_last_error(), untouched

    st, msg, untouched = call(counts, off)
    assert st == L.OK and not untouched
    bad = counts.copy()
    bad[40] = 65
    st, msg, untouched = call(bad, off)
    assert st == L.E_INVALID_ARG and b"rec_counts" in msg and untouched
    bad[40] = -1
    assert call(bad, off)[0] == L.E_INVALID_ARG
    bad = off.copy()
    bad[33], bad[34] = bad[34] + 1, bad[33]
    assert bad[33] > bad[34]
    st, msg, untouched = call(counts, bad)
    assert st == L.E_INVALID_ARG and b"rel_offsets" in msg and untouched
    bad = off.copy()
    bad[-1] += 1                                            # beyond n_rel
    st, msg, untouched = call(counts, bad)
    assert st == L.E_INVALID_ARG and b"rel_offsets" in msg and untouched
    with pytest.raises(pkg.IllegalArgumentException):
        pkg.prep.evaluate_ranked(dev(rec), dev(counts), dev(bad), dev(rel), [3])
