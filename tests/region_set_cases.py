"""The region sets of the reference's builder mains (PlaceVisits.scala:50-87) restated with numpy, and seeded inputs
shared by the CPU tests (restatement against hand-written cases) and the GPU tests (device against restatement)."""
import itertools

import numpy as np

import prep_cases

PLACE_VISIT_COLUMNS = ("person_id", "timestamp", "place_id", "region_id", "category_id")
MS_PER_DAY = 86_400_000
TILE = 2048          # output rows of one block of rs_merge_gather (csrc/region_sets.hip)
RUN_LENGTHS = [(0, 0), (1, 0), (0, 1), (1, 1), (2047, 1), (2048, 0), (1024, 1024), (2049, 2047), (4097, 3)]
INTERLEAVINGS = ("alternating", "a_first", "b_first", "random")
REGION_A, REGION_B, REGION_EMPTY, REGION_UNLISTED = 10, 20, 15, 99   # 15 is listed and has no rows


# ---- the restatement -------------------------------------------------------------------------------------------------

def max_timestamp(timestamps):
    return int(np.max(np.asarray(timestamps, np.int64)))       # raises on no visits, as the reference fails there


def extract_region_ids(region_ids):
    return np.unique(np.asarray(region_ids, np.int64))         # distinct, ascending


def region_sets(region_ids):
    """regionIds.map(Seq(_)) ++ regionIds.combinations(2) (PlaceVisits.scala:64-65)."""
    ids = [int(r) for r in region_ids]
    return [(r,) for r in ids] + list(itertools.combinations(ids, 2))


def set_rows(row_regions, region_set):
    """Row numbers of where(region_id === a or region_id === b), in input order."""
    r = np.asarray(row_regions, np.int64)
    mask = np.zeros(len(r), bool)
    for reg in region_set:
        mask |= r == int(reg)
    return np.flatnonzero(mask)


def partition(row_regions, region_ids):
    """(rows, offsets) of locrec_region_partition: rows grouped by the rank of their region in the ascending
    region_ids, ascending inside a group, the rows of unlisted regions last."""
    r = np.asarray(row_regions, np.int64)
    ids = np.asarray(region_ids, np.int64)
    groups = [np.flatnonzero(r == reg) for reg in ids] + [np.flatnonzero(~np.isin(r, ids))]
    offsets = np.zeros(len(ids) + 2, np.int64)
    np.cumsum([len(g) for g in groups], out=offsets[1:])
    return np.concatenate(groups).astype(np.int32), offsets


def place_visits_of_set(place_visits, region_set):
    rows = set_rows(place_visits["region_id"], region_set)
    return {k: np.asarray(place_visits[k], np.int64)[rows] for k in PLACE_VISIT_COLUMNS}


def visits_from_fixed_offset(max_timestamp_ms, last_days_count):
    """At a fixed UTC offset a wall-clock day is 86,400,000 ms whatever the offset."""
    return int(max_timestamp_ms) - int(last_days_count) * MS_PER_DAY


# ---- inputs ----------------------------------------------------------------------------------------------------------

HAND_REGIONS = np.array([7, 3, 5, 3, 3, 7, 5, 42, 3, 7, 5, 5], np.int64)      # 3 regions + one row of an unlisted one
HAND_SET_ROWS = {(3,): [1, 3, 4, 8], (5,): [2, 6, 10, 11], (7,): [0, 5, 9], (3, 5): [1, 2, 3, 4, 6, 8, 10, 11],
                 (3, 7): [0, 1, 3, 4, 5, 8, 9], (5, 7): [0, 2, 5, 6, 9, 10, 11]}
HAND_PARTITION = ([1, 3, 4, 8, 2, 6, 10, 11, 0, 5, 9, 7], [0, 4, 8, 11, 12])


def table_for(regions, seed=0):
    """Five int64 place-visit columns whose values name their row, around the given region column."""
    rng = np.random.default_rng(seed)
    n = len(regions)
    row = np.arange(n, dtype=np.int64)
    return {"person_id": 2040 + row * 7, "timestamp": 1_600_000_000_000 + rng.integers(0, 90 * MS_PER_DAY, n),
            "place_id": 40 + (row * 13) % 1000, "region_id": np.asarray(regions, np.int64), "category_id": -5 + row % 20}


def run_case(la, lb, how, seed=0):
    """A region column with `la` rows of REGION_A and `lb` of REGION_B interleaved as `how` says, rows of an unlisted
    region at the head, at the tail and scattered between (every 97th row and around the tile limits of the merge),
    and no row of REGION_EMPTY.  -> (regions, listed region ids ascending)."""
    rng = np.random.default_rng(seed)
    if how == "alternating":
        m = min(la, lb)
        ab = np.empty(2 * m, np.int64)
        ab[0::2], ab[1::2] = REGION_A, REGION_B
        ab = np.concatenate([ab, np.full(la - m, REGION_A, np.int64), np.full(lb - m, REGION_B, np.int64)])
    elif how == "a_first":
        ab = np.concatenate([np.full(la, REGION_A, np.int64), np.full(lb, REGION_B, np.int64)])
    elif how == "b_first":
        ab = np.concatenate([np.full(lb, REGION_B, np.int64), np.full(la, REGION_A, np.int64)])
    else:
        ab = rng.permutation(np.concatenate([np.full(la, REGION_A, np.int64), np.full(lb, REGION_B, np.int64)]))
    between = set(range(96, len(ab), 97)) | {p for p in (TILE - 1, TILE, TILE + 1, 2 * TILE) if 0 < p < len(ab)}
    at = [0] + sorted(between) + [len(ab)]
    regions = np.insert(ab, at, REGION_UNLISTED)
    return regions, np.array([REGION_A, REGION_EMPTY, REGION_B], np.int64)


def many_regions_case(seed, n=70_000, n_regions=7):
    """n rows over n_regions listed regions of very different sizes (negative ids among them) and one unlisted."""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.choice(np.arange(-50, 50), n_regions, replace=False)).astype(np.int64)
    weights = np.r_[np.arange(1, n_regions + 1) ** 2.0, 3.0]
    pick = rng.choice(n_regions + 1, n, p=weights / weights.sum())
    regions = np.where(pick < n_regions, ids[np.minimum(pick, n_regions - 1)], 1000).astype(np.int64)
    return regions, ids


def builder_case(seed=11, n_places=60, n_visits=600):
    """The two sample tables of a builder main: prep_cases.join_case over its three regions (-5, 2, 9)."""
    return prep_cases.join_case(seed, n_places=n_places, n_visits=n_visits)
