"""The device build of the stochastic graph's layout (csrc/sg_create_device.hip) at the limits of its piece plan, its two
radix sorts and its id table: the graphs of tests/sg_build_limit_cases.py, each the smallest that stands on its limit
(tests/test_sg_build_limit_cases.py asserts that it does).

Every case goes through compare() of tests/test_gpu_sg_device_build.py: host-built and device-built handle under the
same environment, `facts` equal, every request bit-equal, the batch byte-equal, and the device-built result against the
oracle at that file's bar (ids, iteration counter and converged flag equal, probabilities rtol = 1e-6).  On top of that
the handles' vertices / edges / live_count / weight_dictionary / device_sweep_bytes must be what plan() derives from
DESIGN.md section 4 - compare() has asserted the two handles' facts equal, so the figures hold for both, and two
builders that agree on a wrong plan do not pass.

Each docstring names the one-line misreading of the builder that the case bites, argued from the code: a wrong plan or
id range writes outside the layout or the table, so no mutated builder is ever run."""
import numpy as np
import pytest

import sg_build_limit_cases as limits
from test_gpu_sg_device_build import compare

pytestmark = pytest.mark.gpu

NO_DENSE, NO_COL16, NO_DICT = "LOCREC_SG_NO_DENSE_IDS", "LOCREC_SG_NO_COL16", "LOCREC_SG_NO_DICT"


def check(pkg, oracle, monkeypatch, c, env=None, requests=None):
    """compare() under `env`, then both handles' facts against plan().  -> (facts, plan)"""
    p = limits.plan(c["source"], c["target"], c["weight"])
    if env:
        monkeypatch.setenv(env, "1")
    f = compare(pkg, oracle, c["source"], c["target"], c["weight"], c["requests"] if requests is None else requests)
    dictionary = 0 if env == NO_DICT else p["weight_dictionary"]
    expect = dict(vertices=p["vertices"], edges=p["edges"], live_count=p["live"], weight_dictionary=dictionary,
                  device_sweep_bytes=limits.sweep_bytes(p, use16=p["use16"] and env != NO_COL16, dictionary=dictionary > 0))
    assert {k: f[k] for k in expect} == expect, c["limit"]      # (facts(host) == facts(device): asserted by compare)
    return f, p


def memory_returned(pkg, run):
    from locations_recommender_amd import _lib as L
    before = L.device_bytes_in_use()
    run()
    assert L.device_bytes_in_use() == before


# ---- 1. remainder classes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", [None, NO_DENSE, NO_COL16])
def test_class_spill(pkg, oracle, monkeypatch, env):
    """Every class's segment number k = 64 >> c, the first of its second piece; in classes 0 .. 5 that row also owns one
    or two full pieces, in class 6 three (the long area).
    Bites: sg_db_row_maps' rem_slot0 without the `k / per` term - the spilled row lands on segment 0 of the class's
    FIRST piece, over the weights of the class's first row, and both rows answer differently from the host build and
    the oracle; sg_db_pinfo without `(p - piece_begin[c])` (or without its factor `64 >> c`) - the second piece of the
    class reports the first piece's parts (or part_begin[c] + 1), so the sweep stores the spilled row's sum through the
    seg_out entry of the class's first (second) row and the spilled row keeps no remainder at all.  Neither can show
    for c = 1 .. 5 in the older graphs, whose classes 1 .. 5 have two rows.  LOCREC_SG_NO_DENSE_IDS ranks the same
    vertices by the sort, LOCREC_SG_NO_COL16 writes the same slots as int32 columns."""
    check(pkg, oracle, monkeypatch, limits.class_spill(), env)


def test_class_exact(pkg, oracle, monkeypatch):
    """Every class is exactly one piece and every segment has an owner.  Bites: a piece count of `rows / per + 1` instead
    of the ceiling - one piece and 64 >> c parts too many in EVERY class, which plan()'s pieces and parts show in
    device_sweep_bytes even when both builders agree (the older graphs fill no class exactly)."""
    check(pkg, oracle, monkeypatch, limits.class_exact())


@pytest.mark.parametrize("odd", [True, False])
def test_classes_alternate(pkg, oracle, monkeypatch, odd):
    """Empty classes: an empty class begins at the same piece and the same part as the populated class below it, so
    sg_db_pinfo's chain `p >= piece_begin[k]` meets ties, which it must resolve towards the LOWER class.
    Bites: the same chain with `>` - the first piece of every class goes to a class above it (in the odd variant the
    second of class 3's two pieces keeps class 3, its first does not) - or any resolution that prefers the higher class
    at equal begins, such as a bisection for the first begin <= p in the descending array: the piece gets an empty
    class's wider segments, the butterfly adds several rows into one partial, and `part` is computed with the wrong
    `64 >> c`.  The older graphs populate all seven classes, or one."""
    check(pkg, oracle, monkeypatch, limits.classes_alternate(odd))


# ---- 2. whole pieces, the long area, no dead slot ---------------------------------------------------------------

def test_whole_piece_rows(pkg, oracle, monkeypatch):
    """256, 512, 768, 2048, 2304 and 2560 edges exactly: no row has a remainder, so np == npart == the 33 full pieces,
    sg_db_pinfo never leaves its first branch, no slot is padding, and the long area holds rows of exactly kLongRow
    and kLongRow + 1 full pieces whose lrows entry says "no remainder".
    Bites: a plan that gives every class at least one piece (`max(1, pieces)`), or one more piece "for the padding" -
    pieces and parts are plan()'s, through device_sweep_bytes; a weight buffer whose untouched slots are counted - the
    dictionary must hold the 12 edge weights and no +0.0 (a build that always appends it reports 13); `rem_part`'s -1
    used as an index for a row without remainder - here EVERY row takes that branch, and a stray write to seg_out[-1]
    or to the slot behind a long row's run would meet a neighbour that a sweep really reads."""
    c = limits.whole_piece_rows()
    f, p = check(pkg, oracle, monkeypatch, c)
    assert f["weight_dictionary"] == len(np.unique(c["weight"])) == limits.WHOLE_WEIGHTS
    assert p["pieces"] * 256 == p["edges"]


def test_long_rows_only(pkg, oracle, monkeypatch):
    """n_short == 0: the counters in front of row n_short are sc[0] (all zero), long_base is 3 T, sg_db_live ranks every
    row from the high half of its scan word, lrows has T entries and sg_finalize's loop over the short rows has none.
    Bites: `l >= n_short` as `l > n_short` in sg_db_row_maps - row 0 would take a short row's three slots for its four
    full pieces and get no lrows entry, so nobody finalises it; `n_short + (sc[v] >> 32)` with the halves of the word
    taken the other way round - every row would get live index 0.  Both show as answers that differ from the host
    build's and the oracle's (requests: both ends, two rows, source-only vertices)."""
    _, p = check(pkg, oracle, monkeypatch, limits.long_rows_only())
    assert p["n_short"] == 0


def test_closed_graph(pkg, oracle, monkeypatch):
    """No source-only vertex: nd == 0, the dead-slot sort is skipped and sg_db_dead_ptr bisects an empty list.  Bites:
    a bisection that reads dk[0] before it looks at nd (the one-element allocation is uninitialised: dead_ptr would
    not be all zero and a request would patch slots it does not own); a temporary of the skipped steps that is not
    freed (device_bytes_in_use)."""
    c = limits.closed_graph()

    def run():
        _, p = check(pkg, oracle, monkeypatch, c)
        assert p["source_only"] == 0
    memory_returned(pkg, run)


# ---- 3. vertex counts -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", limits.TINY_KINDS)
def test_tiny(pkg, oracle, monkeypatch, kind):
    """One or two vertices, one or two edges: nv == 1 (db_bits(1) must still be a bit: a radix sort over [0, 0) bits
    may leave its output unwritten), a mark table of one entry plus its closing 0 (nv is read from r[1]), T == 1, one
    piece of which 254 or 255 slots are padding, and a source-only vertex whose whole dead list is one slot.
    Bites: a table sized id_span instead of id_span + 1 (no entry at all for the self-loop); the same (source, target)
    pair twice collapsed into one slot by a scatter keyed on the pair instead of the sorted position - the
    double self-loop would weigh 0.75 or 0.25 instead of 1, and `edges` would still say 2."""
    memory_returned(pkg, lambda: check(pkg, oracle, monkeypatch, limits.tiny(kind)))


@pytest.mark.parametrize("nv", limits.VERTEX_COUNTS)
def test_vertex_count(pkg, oracle, monkeypatch, nv):
    """db_bits(nv) sizes both radix sorts.  At nv = 2^k (2, 4, 256) and 2^k - 1 (255) the upper half of the vertices has
    the highest of the k bits, the top row in the sort by target and the second-highest vertex in the sort of the dead
    slots by source among them.
    Bites: a bit count of floor(log2(nv)) or ceil_log2(nv - 1)-style arithmetic that is one short at these counts: the
    stable sort files vertex v + 2^(k-1) under v, the two rows' edges interleave in edge-list order, sg_db_row_bounds
    keeps the last fragment of each and the in-degrees, T or the slots differ from the host's and plan()'s; in the dead
    sort the keys are then not ascending and sg_db_dead_ptr's bisection gives the second-highest vertex another
    vertex's slots, so its request (asked twice, the lowest vertex in between) differs.  nv = 3, 5, 257 are built for
    vertices / live_count here and bite in test_vertex_count_with_both_ends_in_one_sort."""
    check(pkg, oracle, monkeypatch, limits.vertex_count(nv))


@pytest.mark.parametrize("ends", limits.VERTEX_ENDS)
@pytest.mark.parametrize("nv", limits.VERTEX_END_COUNTS)
def test_vertex_count_with_both_ends_in_one_sort(pkg, oracle, monkeypatch, nv, ends):
    """nv = 2^k + 1: vertex 2^k alone has bit k.  Bites: db_bits' `(1 << b) < n` as `(1 << b) < n - 1` (k bits for
    2^k + 1 keys): the highest vertex is filed under key 0.  "rows": vertex 0 is a row too, so the in-edges of both
    interleave, sg_db_row_bounds keeps one fragment of each row and the edges of the other fragments are scattered by
    the wrong row start (the bounds check of sg_db_scatter or the comparison with the host build fails).  "sources":
    vertex 0 is a source-only vertex too, the sorted dead keys read 0, 2^k, 0, ... and sg_db_dead_ptr's bisection is
    wrong for both vertices, which are the requests.  With the issue's roles (test_vertex_count) key 0 is absent from
    both sorts and the misfiled key stays contiguous: harmless, which is why these two relabelled graphs exist."""
    check(pkg, oracle, monkeypatch, limits.vertex_count(nv, ends))


# ---- 4. the id range --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ne", [262144, 262145])
def test_stride(pkg, oracle, monkeypatch, ne):
    """sg_db_minmax runs at most 1024 blocks of 256 threads: 262,144 edges a trip.  The smallest and the largest id
    stand in the LAST edge alone, so at 262,145 edges both ends of the range are the second trip's work and at 262,144
    the last thread's of the first trip.
    Bites: the loop read as an `if`, or a stride of gridDim.x without the block size (thread t then re-reads edges
    below 262,144 and never reaches the last one): the range misses id 0 and the largest id, sg_db_mark's index for
    that edge lies in front of and behind the table.  That is a fault, not a wrong answer, which is why the loop is
    read and not mutated; what this case adds is a build whose range, vertex count (plan()'s) and table come from the
    second trip.  At 262,144 the same edge is the last thread's of the last block of a full first trip: a bound of
    `e < ne - 1` loses it there."""
    check(pkg, oracle, monkeypatch, limits.stride(ne))


@pytest.mark.parametrize("env", [None, NO_DENSE])
@pytest.mark.parametrize("kind", limits.ID_END_KINDS)
def test_id_ends(pkg, oracle, monkeypatch, kind, env):
    """`low` / `high`: the table path with id_lo == INT64_MIN and with a table that ends at INT64_MAX.  Bites: `id - lo`
    or `lo + i` in signed arithmetic (sg_db_mark, sg_db_dense_rank, sg_db_dense_vid: the code's run in uint64, where the
    wrap is defined and exact); the sign flip of db_key applied once only (h[0] used as id_lo without flipping back:
    every index is off by 2^63).
    `both`: span 2^64 - 1.  Bites: the span test as `id_span + 1 <= 8 E + 2^20` - span + 1 wraps to 0 and a table of
    one entry is chosen for 334 vertices.
    `table_last` / `sort_first`: spans 8 E + 2^20 - 1 and 8 E + 2^20 with E = 3.  Bites: `(uint64_t)(8 * ne) + (1u <<
    20)` with another constant or `<=`: the paths give the same handle, so this pair shows only that either side of
    the threshold builds the same graph, the table of 1,048,600 entries for three edges included.
    Under LOCREC_SG_NO_DENSE_IDS every kind takes the 64-bit sort and sg_db_bisect's SIGNED comparison: an unsigned one
    would rank INT64_MIN last."""
    check(pkg, oracle, monkeypatch, limits.id_ends(kind), env)


# ---- 5. the two format limits, stood on by the device builder ---------------------------------------------------

@pytest.mark.parametrize("t_plus_2", [65535, 65536, 65537])
def test_uint16_limit_from_device(pkg, oracle, monkeypatch, t_plus_2):
    """The graph of test_gpu_sg_limits.test_uint16_columns_at_their_limit through from_device.  Bites: the device
    builder's restated `T + 2 <= 65536` read as `<= 65537` (uint16 columns at T = 65535: sg_db_fill's `(unsigned
    short)T` still fits, but the batch's first private row T + 1 = 65536 wraps to column 0) or as `<= 65535` (the
    middle graph builds int32 columns: its sweep bytes equal the switched-off form's) - either way the facts differ
    from the host handle's and from plan()'s."""
    c = limits.uint16_limit(t_plus_2)
    targets = [int(v) for v in c["requests"][:6]]                      # persons, row 5, the last row T - 1, row 0
    on, p = check(pkg, oracle, monkeypatch, c, requests=targets)
    off, _ = check(pkg, oracle, monkeypatch, c, NO_COL16, requests=targets[:2])
    assert on["live_count"] == t_plus_2 - 2
    if t_plus_2 <= 65536:
        assert on["device_sweep_bytes"] < off["device_sweep_bytes"], "uint16 columns were not used at T + 2 <= 65536"
    else:
        assert on["device_sweep_bytes"] == off["device_sweep_bytes"], "uint16 columns cannot address T + 1 = 65536"


@pytest.mark.parametrize("distinct", [8191, 8192, 8193])
def test_dictionary_limit_from_device(pkg, oracle, monkeypatch, distinct):
    """The graph of test_gpu_sg_limits.test_weight_dictionary_at_its_limit through from_device.  Bites: db_dictionary's
    restated `nu <= kDictMax` read as `<` (no dictionary at 8192) or a table of 8193 (its last value lies behind the
    64 KB the sweep copies into LDS); a device build whose padding slots are not +0.0 bits (w2 not cleared before the
    scatter): the count of distinct slot weights is not the edge weights + 1."""
    c = limits.dictionary_limit(distinct)
    targets = [int(v) for v in c["requests"][:4]] + [int(c["requests"][-1]), int(c["requests"][0])]
    on, p = check(pkg, oracle, monkeypatch, c, requests=targets)
    off, _ = check(pkg, oracle, monkeypatch, c, NO_DICT, requests=targets[:2])
    assert off["weight_dictionary"] == 0
    assert on["weight_dictionary"] == (distinct if distinct <= 8192 else 0), "the dictionary holds 8192 values, +0.0 included"
    assert (on["device_sweep_bytes"] < off["device_sweep_bytes"]) == (distinct <= 8192)
