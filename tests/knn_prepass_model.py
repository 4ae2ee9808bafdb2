"""A numpy model of the contract of the KNN hit pre-pass (csrc/knn_ht_prepass.h: ht_tile_bases + ht_build_hits).

For a data set (the dictionary make_index takes), a head width H and a list of query rows the model gives what the
pre-pass must leave behind, per query tile of 16:

  tile_base   first hit word of the tile; the closing entry is the batch's total
  off         start of every candidate slice inside the tile's hits; the closing entry is the tile's total
  hits        for every slice the MULTISET of hit words  lane << 21 | q << 16 | product  (the order inside a slice
              is free): a posting of tail place p at candidate row r with value v is one hit for every query q of the
              tile that holds p with value u - (r & 63, q, v * u) in slice r >> 6

Rows are the index's rows: the index sorts the persons by (place count, category count, head count), stably
(index_order), and the H most frequent places - ties by place number - are the head, every other place is a tail place.

The model also computes the documented sub-range width and segment size of a tile and, from them, the route every
sub-range takes (empty / staged / full / overflow), so that a test can assert which paths of the kernel its data reach."""
import numpy as np

QT = 16
WIDTH_MAX = 512
STAGE_MIN, STAGE_SMALL, STAGE_DEFAULT, STAGE_MAX = 64, 4096, 8192, 8192


def width(stage, slices, total):
    """The sub-range width of a tile: the power of two nearest, in ratio, to the slices that hold stage / 2 hits."""
    target = (stage // 2) * slices // max(total, 1)
    w = 1
    while w < WIDTH_MAX and w * 10 <= target * 7:
        w *= 2
    return w


def segment(total, w, slices, entries):
    """Lanes of a wave step that load consecutive postings of ONE entry: the power of two (4 .. 64) that holds twice the
    postings an entry has in a sub-range on average."""
    per_entry2 = 2 * total * w // (slices * max(entries, 1))
    seg = 4
    while seg < 64 and seg < per_entry2:
        seg *= 2
    return seg


def effective_stage(value):
    """Hits of the LDS stage for a LOCREC_KNN_HT_PRE_STAGE value (None: unset)."""
    return STAGE_DEFAULT if value is None else min(STAGE_MAX, max(STAGE_MIN, int(value)))


def records_per_thread(stage):
    """The instantiation ht_build_hits<16, RECS> a stage selects."""
    return 8 if stage <= STAGE_SMALL else 16


def head_mask(d, head):
    """True for the `head` most frequent places (stable: ties go to the lower place number)."""
    freq = np.bincount(d["p_idx"], minlength=d["p_dim"])
    by_freq = np.argsort(-freq, kind="stable")
    mask = np.zeros(d["p_dim"], bool)
    mask[by_freq[:head]] = True
    return mask


def index_order(d, head):
    """order[r] = input position of the person in row r of the index."""
    hm = head_mask(d, head)
    n = len(d["person_ids"])
    pc, cc = np.diff(d["p_rowptr"]), np.diff(d["c_rowptr"])
    is_head = hm[d["p_idx"]].astype(np.int64)
    hc = np.add.reduceat(np.append(is_head, 0), d["p_rowptr"][:-1]) * (pc > 0) if n else np.zeros(0, np.int64)
    return np.lexsort((np.arange(n), hc, cc, pc))


class Prepass:
    """The model's answer for one batch; see the module's docstring.  `tile`, `slice` and `word` list every hit, sorted
    by (tile, slice, word)."""

    def __init__(self, slices, ntiles, tile, slice_, word, entries, entry_rows):
        self.slices, self.ntiles = slices, ntiles
        self.tile, self.slice, self.word = tile, slice_, word
        self.entries = entries          # per tile: its (query, tail place) pairs
        self.entry_rows = entry_rows    # per tile: for every entry the candidate rows of its place (a list of arrays)
        self.counts = np.zeros((ntiles, slices), np.int64)
        np.add.at(self.counts, (tile, slice_), 1)
        self.tile_base = np.concatenate([[0], np.cumsum(self.counts.sum(axis=1))]).astype(np.int64)
        self.off = np.concatenate([np.zeros((ntiles, 1), np.int64), np.cumsum(self.counts, axis=1)], axis=1).astype(np.uint32)

    def slice_words(self, t, s):
        a = self.tile_base[t] + int(self.off[t, s])
        return self.word[a:a + self.counts[t, s]]

    def subranges(self, t, stage):
        """[(first slice, slices, hits, route)] of tile t under a stage of `stage` hits."""
        w = width(stage, self.slices, int(self.counts[t].sum()))
        out = []
        for s0 in range(0, self.slices, w):
            n = int(self.counts[t, s0:s0 + w].sum())
            route = "empty" if n == 0 else "overflow" if n > stage else "full" if n == stage else "staged"
            out.append((s0, min(w, self.slices - s0), n, route))
        return out

    def segment(self, t, stage):
        total = int(self.counts[t].sum())
        return segment(total, width(stage, self.slices, total), self.slices, int(self.entries[t]))

    def max_entry_postings(self, t, stage):
        """The most postings one entry of tile t has inside one sub-range."""
        w = width(stage, self.slices, int(self.counts[t].sum()))
        return max((int(np.bincount((rows >> 6) // w).max()) for rows in self.entry_rows[t] if len(rows)), default=0)

    def misalignments(self, t, stage):
        """(tile_base + run) & 3 of every staged or full sub-range of tile t."""
        run, out = int(self.tile_base[t]), []
        for _, _, n, route in self.subranges(t, stage):
            if route in ("staged", "full"):
                out.append(run & 3)
            run += n
        return out

    def routes(self, stage):
        """{route: number of sub-ranges} over all tiles."""
        out = {"empty": 0, "staged": 0, "full": 0, "overflow": 0}
        for t in range(self.ntiles):
            for _, _, _, route in self.subranges(t, stage):
                out[route] += 1
        return out


def prepass(d, order, head, qrows, keep_entries=True):
    """The model for the query rows `qrows` (rows of the index, in batch order) of data set d under head width `head`;
    order = index_order(d, head), or the order read from the handle."""
    order = np.asarray(order)
    n = len(order)
    slices = (n + 63) // 64
    row_of_input = np.empty(n, np.int64)
    row_of_input[order] = np.arange(n)
    tail = ~head_mask(d, head)
    # postings of the tail places: (row, value), rows ascending inside a place
    e_row = row_of_input[np.repeat(np.arange(n), np.diff(d["p_rowptr"]))]
    e_place, e_val = d["p_idx"].astype(np.int64), d["p_val"].astype(np.int64)
    sel = tail[e_place]
    by = np.lexsort((e_row[sel], e_place[sel]))
    p_place, p_row, p_val = e_place[sel][by], e_row[sel][by], e_val[sel][by]
    p_ptr = np.searchsorted(p_place, np.arange(d["p_dim"] + 1))
    ntiles = (len(qrows) + QT - 1) // QT
    tiles, slices_, words = [], [], []
    entries = np.zeros(ntiles, np.int64)
    entry_rows = [[] for _ in range(ntiles)]
    for j, r in enumerate(qrows):
        i = order[r]
        for e in range(d["p_rowptr"][i], d["p_rowptr"][i + 1]):
            p = int(d["p_idx"][e])
            if not tail[p]:
                continue
            t, q, u = j // QT, j % QT, int(d["p_val"][e])
            rows, vals = p_row[p_ptr[p]:p_ptr[p + 1]], p_val[p_ptr[p]:p_ptr[p + 1]]
            entries[t] += 1
            if keep_entries:
                entry_rows[t].append(rows)
            tiles.append(np.full(len(rows), t, np.int64))
            slices_.append(rows >> 6)
            words.append(((rows & 63) << 21) | (q << 16) | (vals * u))
    if tiles:
        tile, slice_, word = np.concatenate(tiles), np.concatenate(slices_), np.concatenate(words)
    else:
        tile = slice_ = word = np.zeros(0, np.int64)
    by = np.lexsort((word, slice_, tile))
    return Prepass(slices, ntiles, tile[by], slice_[by], word[by].astype(np.uint32), entries, entry_rows)


def brute_force(d, order, head, qrows):
    """The same answer from a plain loop over tiles, queries, candidate rows and places (for small data):
    {(tile, slice): sorted list of hit words}."""
    order = [int(x) for x in order]
    freq = [0] * d["p_dim"]
    for p in d["p_idx"]:
        freq[int(p)] += 1
    ranked = sorted(range(d["p_dim"]), key=lambda p: (-freq[p], p))
    is_head = set(ranked[:head])
    vec = []
    for r in range(len(order)):
        i = order[r]
        vec.append({int(d["p_idx"][e]): int(d["p_val"][e]) for e in range(d["p_rowptr"][i], d["p_rowptr"][i + 1])})
    out = {}
    for j, qr in enumerate(qrows):
        for r in range(len(order)):
            for p, v in vec[r].items():
                if p not in is_head and p in vec[qr]:
                    out.setdefault((j // QT, r >> 6), []).append(((r & 63) << 21) | ((j % QT) << 16) | (v * vec[qr][p]))
    return {k: sorted(v) for k, v in out.items()}


def check_view(view, model, label=""):
    """Compare what KnnIndex.ht_last_hits() returned with the model: tile_base and every off entry exactly, the hit
    words as a sorted multiset per tile and slice."""
    assert view["query_tile"] == QT and view["tiles"] == model.ntiles, (label, view["query_tile"], view["tiles"])
    assert view["slice0"] == 0 and view["nslices"] == model.slices, (label, view["slice0"], view["nslices"])
    assert np.array_equal(view["tile_base"], model.tile_base), (label, "tile_base")
    bad = np.argwhere(view["off"] != model.off)
    assert bad.size == 0, (label, "off differs at (tile, slice)", bad[:8].tolist())
    hits = view["hits"]
    assert len(hits) == len(model.word), (label, len(hits), len(model.word))
    segment_of = model.tile * model.slices + model.slice   # the (tile, slice) every position of `hits` belongs to
    got = hits[np.lexsort((hits, segment_of))]
    bad = np.flatnonzero(got != model.word)
    assert bad.size == 0, (label, "hit words differ, first at (tile, slice)",
                           [(int(model.tile[i]), int(model.slice[i]), hex(int(got[i])), hex(int(model.word[i]))) for i in bad[:4]])
