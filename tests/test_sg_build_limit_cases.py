"""tests/sg_build_limit_cases.py on the CPU: plan() gives the hand-derived numbers of sg_build_cases.layout_graph(), and
every case stands where its `limit` says - a case that does not reach the limit it is named for would pass on the GPU
without testing anything."""
import numpy as np
import pytest

import sg_build_cases as cases
import sg_build_limit_cases as limits

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max

ALL_CASES = ([("class_spill", ()), ("class_exact", ()), ("classes_alternate", (True,)), ("classes_alternate", (False,)),
              ("whole_piece_rows", ()), ("long_rows_only", ()), ("closed_graph", ())]
             + [("tiny", (k,)) for k in limits.TINY_KINDS] + [("vertex_count", (n,)) for n in limits.VERTEX_COUNTS]
             + [("vertex_count", (n, e)) for n in limits.VERTEX_END_COUNTS for e in limits.VERTEX_ENDS]
             + [("stride", (n,)) for n in (262144, 262145)] + [("id_ends", (k,)) for k in limits.ID_END_KINDS]
             + [("uint16_limit", (65536,)), ("dictionary_limit", (8192,))])


@pytest.fixture(scope="module", autouse=True)
def package(pkg):
    """The generators draw from the package's synth.splitmix64."""


def planned(c):
    return limits.plan(c["source"], c["target"], c["weight"])


def ids_of(c):
    return np.unique(np.concatenate([c["source"], c["target"]]))


def test_plan_of_the_layout_graph_by_hand():
    """DEGREES: class 0 = 1, 4, the rem 1 of 257 / 513 / 769 / 2049, the rem 3 of 2307 and the 70 small rows = 77; classes
    1 .. 5 both ends once; class 6 = 129, 255 and the rem 255 of 511 and 767; full pieces 1+1+1+1+2+2+2+2+3+3+8+9 = 32
    (... 256, 257, 511 / 512, 513, 767 / 768, 769 / 2049 / 2307); pieces 32 + 2 + 5 x 1 + 4; parts 32 + 2 x 64 + 32 + 16 +
    8 + 4 + 2 + 4."""
    g = cases.layout_graph()
    p = limits.plan(g["source"], g["target"], g["weight"])
    assert (p["live"], p["n_short"], p["edges"]) == (94, 90, 9648)
    assert p["rows_per_class"] == [77, 2, 2, 2, 2, 2, 4]
    assert (p["nfull_total"], p["pieces"], p["parts"], p["wave_rows"]) == (32, 43, 226, 1)
    assert p["use16"] and 0 < p["weight_dictionary"] == p["distinct"] <= 8192
    assert p["device_sweep_bytes"] == 43 * 256 * 4 + 43 * 8 + 226 * 16 + 94 * 16


@pytest.mark.parametrize("name,args", ALL_CASES, ids=lambda x: x if isinstance(x, str) else "-".join(map(str, x)))
def test_cases_are_deterministic_and_well_formed(name, args):
    a, b = getattr(limits, name)(*args), getattr(limits, name)(*args)
    for k in ("source", "target", "weight"):
        assert a[k].dtype == (np.float64 if k == "weight" else np.int64) and a[k].ndim == 1
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), k
    assert len(a["source"]) == len(a["target"]) == len(a["weight"]) > 0
    assert list(a["requests"]) == list(b["requests"]) and isinstance(a["limit"], str) and a["limit"]
    ids = ids_of(a)
    req = [int(v) for v in a["requests"]]
    assert all(v in ids for v in req)
    dead = np.setdiff1d(a["source"], a["target"])
    if name in ("uint16_limit", "dictionary_limit"):                   # (those two keep the targets they always had)
        assert any(v in dead for v in req) and any(v not in dead for v in req)
        return
    assert int(ids[0]) in req and int(ids[-1]) in req
    if len(dead):
        asked = [v for v in req if v in dead]
        assert asked and len(asked) > len(set(asked)), "a source-only vertex is asked twice"
    assert np.all(a["weight"] > 0) and np.all(np.isfinite(a["weight"]))


def test_weights_depend_on_term_order():
    """count / total with an odd total: the weights of a source are not dyadic, so a row's sum rounds."""
    c = limits.class_spill()
    w = c["weight"]
    assert np.mean(w * 2.0 ** 30 == np.floor(w * 2.0 ** 30)) < 0.5, "most weights are not multiples of 2^-30"


def test_class_spill():
    c = limits.class_spill()
    p = planned(c)
    assert p["rows_per_class"] == [65, 33, 17, 9, 5, 3, 2] and p["pieces_per_class"] == [2] * 7
    assert p["live"] == 134 and p["edges"] < 10_000 and p["n_short"] == 133 and p["use16"]
    assert p["parts"] == p["nfull_total"] + 2 * (64 + 32 + 16 + 8 + 4 + 2 + 1)
    deg = np.bincount(c["target"], minlength=134)[:134]
    assert np.array_equal(deg // 256, c["nfull"]) and np.sum(deg // 256 == 3) == 1
    for k in range(7):
        members = np.flatnonzero(c["cls_of"] == k)                     # ascending vertex = ascending live order here:
        rem = deg[members] % 256                                       # the one long row is the highest vertex of class 6
        assert set(rem.tolist()) == set(limits.CLASS_ENDS[k]), "both ends of the class"
        assert [limits.ceil_log2((int(r) + 3) // 4) for r in rem] == [k] * len(members)
        spilled = members[-1]                                          # segment number 64 >> k: the second piece's first
        assert len(members) == (64 >> k) + 1 and deg[spilled] // 256 == (3 if k == 6 else 1 + k % 2)
        assert np.any(deg[members[:-1]] // 256 > 0), "a row of the first piece has full pieces too"
        if k < 6:
            assert np.all(deg[members] // 256 <= 2)
    long_row = int(np.flatnonzero(deg // 256 == 3)[0])
    assert c["cls_of"][long_row] == 6 and long_row == np.flatnonzero(c["cls_of"] == 6)[-1]
    assert long_row in c["requests"] and p["source_only"] == limits.SPILL_N_DEAD


def test_class_exact():
    p = planned(limits.class_exact())
    assert p["rows_per_class"] == [64, 32, 16, 8, 4, 2, 1] and p["pieces_per_class"] == [1] * 7
    assert p["parts"] == p["nfull_total"] + p["live"], "every segment has an owner"
    assert p["nfull_total"] == 4 and p["pieces"] == 11


@pytest.mark.parametrize("odd", [True, False])
def test_classes_alternate(odd):
    p = planned(limits.classes_alternate(odd))
    if odd:
        assert p["rows_per_class"] == [0, 3, 0, 9, 0, 3, 0] and p["pieces_per_class"] == [0, 1, 0, 2, 0, 2, 0]
    else:
        assert p["rows_per_class"] == [3, 0, 3, 0, 3, 0, 3] and p["pieces_per_class"] == [1, 0, 1, 0, 1, 0, 3]
    assert p["nfull_total"] == sum(1 for n in p["rows_per_class"] if n) and p["n_short"] == p["live"]


def test_whole_piece_rows():
    c = limits.whole_piece_rows()
    p = planned(c)
    assert sorted(np.bincount(c["target"])[np.unique(c["target"])].tolist()) == list(limits.WHOLE_DEGREES)
    assert p["rows_per_class"] == [0] * 7 and p["pieces"] == p["nfull_total"] == p["parts"] == 33
    assert p["pieces"] * 256 == p["edges"] == 8448 and p["wave_rows"] == 2 and p["n_short"] == 2 and p["live"] == 6
    assert len(np.unique(c["weight"])) == limits.WHOLE_WEIGHTS == 12 and not np.any(c["weight"] == 0.0)
    assert p["distinct"] == p["weight_dictionary"] == 12, "no padding slot: no +0.0 in the dictionary"


def test_long_rows_only():
    c = limits.long_rows_only()
    p = planned(c)
    assert sorted(np.bincount(c["target"])[np.unique(c["target"])].tolist()) == list(limits.LONG_DEGREES)
    assert p["n_short"] == 0 and p["live"] == 4 and p["wave_rows"] == 1 and p["nfull_total"] == 3 + 4 + 8 + 9
    assert p["rows_per_class"] == [3, 0, 0, 0, 0, 0, 0]                 # 769, 2049, 2305: one element over
    assert np.mean(np.isin(c["source"], np.unique(c["target"]))) < 0.2, "fed mostly by source-only vertices"
    assert p["source_only"] == 400


def test_closed_graph():
    c = limits.closed_graph()
    p = planned(c)
    assert p["source_only"] == 0 and p["vertices"] == p["live"] == 300
    assert len(np.setdiff1d(c["source"], c["target"])) == 0
    pairs = c["source"] * 1000 + c["target"]
    assert len(pairs) - len(np.unique(pairs)) >= 40, "repeated (source, target) pairs"


@pytest.mark.parametrize("kind,nv,ne,live", [("self_loop", 1, 1, 1), ("one_edge", 2, 1, 1), ("pair", 2, 2, 2),
                                             ("double_loop", 1, 2, 1), ("two_loops", 2, 2, 2)])
def test_tiny(kind, nv, ne, live):
    c = limits.tiny(kind)
    p = planned(c)
    assert (p["vertices"], p["edges"], p["live"]) == (nv, ne, live)
    assert p["pieces"] == 1 and p["parts"] == 64 and p["rows_per_class"] == [live, 0, 0, 0, 0, 0, 0]
    assert p["distinct"] == len(np.unique(c["weight"])) + 1             # the padding's +0.0
    if kind == "double_loop":
        assert c["weight"].tolist() == [0.25, 0.75] and c["source"].tolist() == c["target"].tolist() == [5, 5]


@pytest.mark.parametrize("nv", limits.VERTEX_COUNTS)
def test_vertex_count(nv):
    c = limits.vertex_count(nv)
    p = planned(c)
    assert p["vertices"] == nv and np.array_equal(ids_of(c), np.arange(nv))
    top, hub = nv - 1, nv - 2
    top_sources = np.unique(c["source"][c["target"] == top])
    assert limits.in_degree(c, top) >= 2 and len(top_sources) >= 2
    assert limits.in_degree(c, 0) == 0 and limits.out_degree(c, 0) >= 2
    if nv > 2:
        assert limits.in_degree(c, hub) == 0 and limits.out_degree(c, hub) >= 3
        hub_rows = len(np.unique(c["target"][c["source"] == hub]))
        assert hub_rows >= {3: 1, 4: 2}.get(nv, 3)
    assert p["source_only"] == (1 if nv == 2 else 2) and p["live"] == nv - p["source_only"]
    bits = limits.ceil_log2(nv)                                         # what both radix sorts must cover
    assert top >> (bits - 1) == 1, "the top row carries the highest bit of the sort by target"
    if nv in (4, 255, 256):
        assert hub >> (bits - 1) == 1, "and the dead slots' source the highest bit of the sort by source"
    if nv in (3, 5, 257):
        assert top == 1 << (bits - 1), "the top index is the only one with the new bit"


def interleaved(where_a, where_b):
    """Edge-list positions of two kinds of edges: neither kind lies wholly in front of the other."""
    a, b = np.flatnonzero(where_a), np.flatnonzero(where_b)
    return len(a) >= 2 and len(b) >= 2 and a.min() < b.max() and b.min() < a.max()


@pytest.mark.parametrize("ends", limits.VERTEX_ENDS)
@pytest.mark.parametrize("nv", limits.VERTEX_END_COUNTS)
def test_vertex_count_with_both_ends_in_one_sort(nv, ends):
    """nv = 2^k + 1: the keys 0 and 2^k, which a sort over k bits cannot tell apart, both occur in the sort by target
    ("rows") or in the sort by source of the dead slots ("sources"), interleaved in the edge list."""
    c = limits.vertex_count(nv, ends)
    p = planned(c)
    s, t = c["source"], c["target"]
    top = nv - 1
    assert p["vertices"] == nv and top == 1 << (limits.ceil_log2(nv) - 1) and p["source_only"] == 2
    if ends == "rows":
        assert interleaved(t == 0, t == top)
        assert limits.in_degree(c, 1) == 0 and limits.in_degree(c, nv - 2) == 0
    else:
        assert limits.in_degree(c, 0) == 0 and limits.in_degree(c, top) == 0
        assert interleaved(s == 0, s == top) and len(np.unique(t[s == top])) >= 3
    assert 0 in c["requests"] and top in c["requests"]


@pytest.mark.parametrize("ne", [262144, 262145])
def test_stride(ne):
    c = limits.stride(ne)
    p = planned(c)
    s, t = c["source"], c["target"]
    ids = ids_of(c)
    assert p["edges"] == ne and limits.STRIDE_TRIP == 262144
    assert (s[-1], t[-1]) == (ids[0], ids[-1]) == (0, limits.STRIDE_ROWS + limits.STRIDE_DEAD + 1)
    assert np.sum(s == ids[0]) + np.sum(t == ids[0]) == 1 and np.sum(s == ids[-1]) + np.sum(t == ids[-1]) == 1
    assert (ne - 1 >= limits.STRIDE_TRIP) == (ne == 262145), "the last edge is the second trip's only one, or the first trip's last"
    assert np.array_equal(ids, np.arange(len(ids))), "dense ids"
    assert p["live"] == limits.STRIDE_ROWS + 1 and all(n > 0 for n in p["rows_per_class"]) and p["wave_rows"] >= 2
    assert p["live"] - p["n_short"] >= 3 and p["source_only"] == limits.STRIDE_DEAD + 1


@pytest.mark.parametrize("kind", limits.ID_END_KINDS)
def test_id_ends(kind):
    c = limits.id_ends(kind)
    p = planned(c)
    ids = ids_of(c)
    lo, hi = int(ids[0]), int(ids[-1])
    span = hi - lo                                                      # (Python integers: no wrap)
    table = span < 8 * p["edges"] + (1 << 20)
    if kind in ("table_last", "sort_first"):
        assert p["edges"] == 3 and p["vertices"] == 3
        assert span == 8 * 3 + (1 << 20) - (1 if kind == "table_last" else 0) and table == (kind == "table_last")
        return
    base = limits.class_spill()
    q = planned(base)
    assert {k: p[k] for k in p} == {k: q[k] for k in q}, "the same plan as class_spill"
    inv = np.unique(np.concatenate([c["source"], c["target"]]), return_inverse=True)[1]
    binv = np.unique(np.concatenate([base["source"], base["target"]]), return_inverse=True)[1]
    assert np.array_equal(inv, binv), "monotone: the same vertex index for every edge end"
    if kind == "low":
        assert lo == I64_MIN and table and np.array_equal(ids - ids[0], ids_of(base) - ids_of(base)[0])
    elif kind == "high":
        assert hi == I64_MAX and table and np.array_equal(ids[-1] - ids, ids_of(base)[-1] - ids_of(base))
    else:
        assert (lo, hi) == (I64_MIN, I64_MAX) and span == 2 ** 64 - 1 and not table
        assert (span + 1) % 2 ** 64 == 0 and np.all(np.abs(ids[1:-1]) <= 1000)
    assert int(ids[0]) in c["requests"] and int(ids[-1]) in c["requests"]


@pytest.mark.parametrize("t_plus_2", [65535, 65536, 65537])
def test_uint16_limit(t_plus_2):
    c = limits.uint16_limit(t_plus_2)
    p = planned(c)
    assert p["live"] + 2 == t_plus_2 and p["use16"] == (t_plus_2 <= 65536)
    assert p["source_only"] == 1500 and sum(p["rows_per_class"]) == p["live"] and p["nfull_total"] == 0


@pytest.mark.parametrize("distinct", [8191, 8192, 8193])
def test_dictionary_limit(distinct):
    c = limits.dictionary_limit(distinct)
    p = planned(c)
    assert len(np.unique(c["weight"])) == distinct - 1 and p["pieces"] * 256 > p["edges"]
    assert p["distinct"] == distinct and p["weight_dictionary"] == (distinct if distinct <= 8192 else 0)
