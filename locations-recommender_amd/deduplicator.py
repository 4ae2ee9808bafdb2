"""The place deduplicator of the reference (deduplicator/PlaceDeduplicator.scala, deduplicator/Levenshtein.scala),
computed by liblocrec.so's kernels (csrc/dedup.hip):

    PlaceDeduplicator(maxPlaceDistanceMeters, maxNameDifference).dropDuplicates   PlaceDeduplicator.scala:13-54
    lev                                                                            Levenshtein.scala:18-57

The confirmed places go into the per-region grid of the visit join, so a place meets only the confirmed places within
the radius; the edit distance runs on those pairs alone, thresholded at maxNameDifference.  There is no CPU fallback.

Names are lower-cased with str.lower() (the host language's own, as the reference uses the JVM's toLowerCase) and
compared as UTF-16 code units, which is what Java's String.charAt sees.  The functions below the class take columns
as numpy arrays or torch CUDA tensors, as prep.py does."""
import ctypes as C

import numpy as np

from . import _lib as L
from .prep import _Cols


def encode_names(names, lower=True, what="names"):
    """CSR of the names: (offsets[n + 1] int64, units uint16), lower-cased first unless lower=False.  A None raises
    and names the row, as the reference's UDF dies of a NullPointerException on a null name."""
    parts = []
    for i, s in enumerate(names):
        if s is None or not isinstance(s, str):
            raise TypeError(f"{what} row {i}: the name is {s!r}, a string is required (the reference throws NullPointerException)")
        parts.append(np.frombuffer((s.lower() if lower else s).encode("utf-16-le"), dtype=np.uint16))
    off = np.zeros(len(parts) + 1, np.int64)
    if parts:
        np.cumsum([len(p) for p in parts], out=off[1:])
    units = np.concatenate(parts).astype(np.uint16) if parts else np.zeros(0, np.uint16)
    return off, units


def _units_col(c, a):
    """A uint16 column: tensors of any 2-byte integer type pass as they are (torch has had uint16 only lately)."""
    if c.device:
        assert a.element_size() == 2, "name units must be 16-bit"
        a = a.contiguous()
        c._keep.append(a)
        return C.c_void_p(a.data_ptr()) if a.numel() else None
    return c.col(a, np.uint16)


def lev_distances(a_offsets, a_units, b_offsets, b_units, max_difference=-1):
    """Levenshtein.lev of n pairs of CSR names (locrec_lev_distances): the exact distances, or with
    max_difference >= 0 min(lev, max_difference + 1) by the kernel the deduplicator uses for that threshold.
    -> int32 array (numpy in, numpy out; CUDA tensors in, CUDA tensor out)."""
    c = _Cols(a_offsets, a_units, b_offsets, b_units)
    n = len(a_offsets) - 1
    assert n >= 0 and len(b_offsets) == n + 1
    args = [c.col(a_offsets, np.int64), _units_col(c, a_units), c.col(b_offsets, np.int64), _units_col(c, b_units)]
    out, outp = c.out(n, np.int32)
    L.check(L.lib().locrec_lev_distances(n, *args, int(max_difference), c.mem, outp))
    return out[:n]


def lev(str1, str2):
    """Levenshtein.lev(str1, str2): the strings as given (no lower-casing), compared by UTF-16 code unit."""
    a, b = encode_names([str1], lower=False, what="str1"), encode_names([str2], lower=False, what="str2")
    return int(lev_distances(a[0], a[1], b[0], b[1])[0])


def find_duplicate_places(places, confirmed, max_meters, max_name_difference, not_same_counts=True):
    """locrec_find_duplicate_places.  places / confirmed: mappings with id, region_id, latitude, longitude,
    name_offsets, name_units (lower-cased CSR, see encode_names), all numpy or all CUDA tensors.
    -> (place_rows, confirmed_rows, name_differences, not_same_counts or None): the pairs that are the same place,
    ordered by (place row, confirmed row), and per place how many rows dropDuplicates' literal join returns."""
    keys = ("id", "region_id", "latitude", "longitude", "name_offsets", "name_units")
    pc, cc = [places[k] for k in keys], [confirmed[k] for k in keys]
    c = _Cols(*pc, *cc)
    n_p, n_c = len(pc[0]), len(cc[0])

    def side(cols):
        return [c.col(cols[0], np.int64), c.col(cols[1], np.int64), c.col(cols[2], np.float64), c.col(cols[3], np.float64),
                c.col(cols[4], np.int64), _units_col(c, cols[5])]
    pa, ca = side(pc), side(cc)
    ns, nsp = c.out(n_p, np.int64) if not_same_counts else (None, None)
    fn = L.lib().locrec_find_duplicate_places
    cap = n_p   # a place is seldom the same as several confirmed places; the count says when a second call is needed
    while True:
        (op, opp), (oc, ocp), (od, odp) = c.out(cap, np.int64), c.out(cap, np.int64), c.out(cap, np.int32)
        cnt = C.c_int64(cap)
        L.check(fn(n_p, *pa, n_c, *ca, float(max_meters), int(max_name_difference), c.mem, opp, ocp, odp, C.byref(cnt), nsp))
        m = cnt.value
        if m <= cap:
            return op[:m], oc[:m], od[:m], (ns[:n_p] if not_same_counts else None)
        cap = m


def find_duplicate_places_stats():
    """What this thread's last find_duplicate_places call did: candidates (pairs within the radius), same pairs, chunks,
    and HIP-event milliseconds of its grid / Levenshtein / compaction phases (locrec_find_duplicate_places_stats)."""
    n = [C.c_int64() for _ in range(3)]
    ms = [C.c_double() for _ in range(3)]
    L.check(L.lib().locrec_find_duplicate_places_stats(*[C.byref(x) for x in n], *[C.byref(x) for x in ms]))
    return dict(candidates=n[0].value, same=n[1].value, chunks=n[2].value, grid_ms=ms[0].value, lev_ms=ms[1].value,
                compact_ms=ms[2].value)


class PlaceDeduplicator:
    """Drop-in mirror of the reference class (PlaceDeduplicator.scala:8-11): frames are pandas DataFrames with the
    columns region_id, id, name, latitude, longitude (`places` may have more)."""

    def __init__(self, maxPlaceDistanceMeters, maxNameDifference):
        self.maxPlaceDistanceMeters = float(maxPlaceDistanceMeters)
        self.maxNameDifference = int(maxNameDifference)

    def _columns(self, frame, other_regions, what):
        region = np.ascontiguousarray(frame["region_id"], np.int64)
        names = list(frame["name"])
        # the UDF sees only joined rows (:38-40): a null name in a region the other frame lacks never reaches it
        joined = np.isin(region, other_regions)
        safe = [s if j or isinstance(s, str) else "" for s, j in zip(names, joined)]
        off, units = encode_names(safe, what=what)
        return dict(id=np.ascontiguousarray(frame["id"], np.int64), region_id=region,
                    latitude=np.ascontiguousarray(frame["latitude"], np.float64),
                    longitude=np.ascontiguousarray(frame["longitude"], np.float64), name_offsets=off, name_units=units)

    def _find(self, places, confirmedPlaces):
        p_regions = np.ascontiguousarray(places["region_id"], np.int64)
        c_regions = np.ascontiguousarray(confirmedPlaces["region_id"], np.int64)
        p = self._columns(places, c_regions, "places")
        c = self._columns(confirmedPlaces, p_regions, "confirmedPlaces")
        return p, c, find_duplicate_places(p, c, self.maxPlaceDistanceMeters, self.maxNameDifference)

    def dropDuplicates(self, places, confirmedPlaces):
        """The reference's literal result (:38-53): the places' columns of every (place, confirmed place of its region
        with another id) pair that is NOT the same place - one row PER PAIR, so a place appears once per confirmed
        place of its region that it does not match, and a place whose region has no confirmed place disappears.  Rows
        come in place-row order (the reference leaves the order undefined)."""
        _, _, (_, _, _, not_same) = self._find(places, confirmedPlaces)
        return places.iloc[np.repeat(np.arange(len(places)), not_same)].reset_index(drop=True)

    def findDuplicates(self, places, confirmedPlaces):
        """Additive: the pairs that are the same place -> frame (id, that_id, name_difference), ordered by
        (place row, confirmed row)."""
        import pandas as pd
        p, c, (prow, crow, diff, _) = self._find(places, confirmedPlaces)
        return pd.DataFrame({"id": p["id"][prow], "that_id": c["id"][crow], "name_difference": diff.astype(np.int32)})

    def withoutDuplicates(self, places, confirmedPlaces):
        """Additive: every place that is the same as NO confirmed place, once each, in input order - the anti-join the
        reference's author intended (its README calls the deduplicator "Not completed yet"; with one confirmed place
        per region dropDuplicates gives exactly this, which is what the reference's test checks)."""
        _, _, (prow, _, _, _) = self._find(places, confirmedPlaces)
        keep = np.ones(len(places), bool)
        keep[prow] = False
        return places.iloc[np.flatnonzero(keep)].reset_index(drop=True)
