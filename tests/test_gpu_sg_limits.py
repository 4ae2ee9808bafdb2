"""The two numeric limits of the SG sweep ("Numeric limits"), stood on exactly:

    uint16 columns      T + 2 <= 65536, T = live vertices (csrc/sg.hip `use16`): column values run to T (the slot of the
                        source-only vertices) and, in a batch, T + 1 (the first private row)
    weight dictionary   at most 8192 distinct edge weights, the +0.0 of the padding slots included (`kDictMax`):
                        a uint16 index per slot instead of the fp64 weight

Both limits are literals here, not read from the library.  Single requests and one batch each against the oracle with
the suite's bars (ids and iteration counter equal, probabilities rtol = 1e-6), and bit-equal to the run with the form
switched off (LOCREC_SG_NO_COL16 / LOCREC_SG_NO_DICT)."""
import numpy as np
import pytest

import sg_build_limit_cases as limits
from test_gpu_sg_batch import ALPHA, RTOL, check_against_single, rows_of, same_bits

pytestmark = pytest.mark.gpu


def check_single_against_oracle(oracle, src, dst, w, got, v, eps, max_it):
    oi, op, oit, oconv = oracle.sg_recommend(src, dst, w, int(v), ALPHA, eps, max_it)
    ids, probs, it, conv = got
    assert np.array_equal(ids, oi) and (it, conv) == (oit, oconv), int(v)
    np.testing.assert_allclose(probs, op, rtol=RTOL, atol=0)


def both_forms(pkg, oracle, monkeypatch, env, src, dst, w, targets, eps=0.01, max_it=20):
    """-> (info with the form on, info with `env` set).  Requests with the form on: oracle + bit-equal to the other."""
    on = pkg.SgGraph(src, dst, w)
    monkeypatch.setenv(env, "1")
    off = pkg.SgGraph(src, dst, w)
    monkeypatch.delenv(env)
    for v in targets[:6]:
        got = on.recommend(int(v), ALPHA, eps, max_it)
        check_single_against_oracle(oracle, src, dst, w, got, v, eps, max_it)
        assert same_bits(got, off.recommend(int(v), ALPHA, eps, max_it)), (env, int(v))
    batch = check_against_single(on, targets, eps, max_it)
    other = off.recommend_batch(targets, ALPHA, eps, max_it)
    assert all(np.array_equal(a, b) for a, b in zip(batch, other)) and batch[2].tobytes() == other[2].tobytes()
    for i in (0, len(targets) - 1):
        check_single_against_oracle(oracle, src, dst, w, rows_of(batch, i), targets[i], eps, max_it)
    infos = on.info(), off.info()
    live = on.live_count()
    on.close()
    off.close()
    return infos, live


@pytest.mark.parametrize("t_plus_2", [65535, 65536, 65537])
def test_uint16_columns_at_their_limit(pkg, oracle, monkeypatch, t_plus_2):
    """Bites: `T + 2 <= 65536` read as `<= 65537` keeps uint16 columns at T = 65535, where the batch's first private row
    T + 1 = 65536 wraps to column 0 (the sweep bytes stay below the int32 form's: asserted first); read as `<= 65535`
    the middle graph loses the form (its sweep bytes equal the int32 form's)."""
    T = t_plus_2 - 2
    c = limits.uint16_limit(t_plus_2)                                   # (tests/sg_build_limit_cases.py)
    src, dst, w, targets, persons = c["source"], c["target"], c["weight"], c["requests"], c["persons"]
    assert (T - 1) in src[T:2 * T] and persons[0] in src[:T]           # columns T - 1 and T are used by real edges
    (on, off), live_count = both_forms(pkg, oracle, monkeypatch, "LOCREC_SG_NO_COL16", src, dst, w, targets)
    assert live_count == T
    if t_plus_2 <= 65536:
        assert on["device_sweep_bytes"] < off["device_sweep_bytes"], "uint16 columns were not used at T + 2 <= 65536"
    else:
        assert on["device_sweep_bytes"] == off["device_sweep_bytes"], "uint16 columns cannot address T + 1 = 65536"


@pytest.mark.parametrize("distinct", [8191, 8192, 8193])
def test_weight_dictionary_at_its_limit(pkg, oracle, monkeypatch, distinct):
    """Bites: `nu <= kDictMax` read as `<` reports no dictionary at 8192; kDictMax = 8193 reports one at 8193, whose
    last value lies behind the 64 KB table of the sweep's LDS."""
    c = limits.dictionary_limit(distinct)                               # (tests/sg_build_limit_cases.py)
    src, dst, w, targets, m = c["source"], c["target"], c["weight"], c["requests"], c["edge_weights"]
    assert len(np.unique(w)) == m and not np.any(w == 0.0)
    (on, off), _ = both_forms(pkg, oracle, monkeypatch, "LOCREC_SG_NO_DICT", src, dst, w, targets)
    assert off["weight_dictionary"] == 0
    assert on["weight_dictionary"] == (distinct if distinct <= 8192 else 0), "the dictionary holds 8192 values, +0.0 included"
    assert (on["device_sweep_bytes"] < off["device_sweep_bytes"]) == (distinct <= 8192)
