"""A numpy restatement of the cudf::distinct contract (include/cudf/stream_compaction.hpp, include/cudf/reduction/distinct_count.hpp):
the checker of the GPU tests.

A column is a HostColumn (values, valid, offset). distinct_indices(cols, keep, nulls_equal, nans_equal) -> the ascending int32 row
indices that survive:
  - rows are compared column by column by their normalised bits (-0 == +0; NaN == NaN when nans_equal);
  - a row with a null in any column (nulls unequal) or a valid NaN in any column (nans unequal) equals no row and survives;
  - first / last: the smallest / largest row of each set of equal rows; none: the rows without an equal row; any: here the first
    (the contract leaves it open; the GPU tests check KEEP_ANY by its keys).
distinct_count_table(cols, nulls_equal) counts the distinct rows with NaN == NaN; distinct_count_column follows
reference distinct_count.cu:190-219."""
import json
import os

import numpy as np

from filtered_join_restatement import _SPECIAL, _rows
from oracle.oracle import NP_OF_TYPE_ID, TYPE_ID, HostColumn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_distinct.json")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def host_table(t):
    """Golden table {types, cols, valid, [offset], [rows]} -> list of HostColumn."""
    out = []
    for i, (ty, vals) in enumerate(zip(t["types"], t["cols"])):
        npt = NP_OF_TYPE_ID[TYPE_ID[ty]]
        off = t.get("offset", [0] * len(t["cols"]))[i]
        end = off + t["rows"] if "rows" in t else len(vals)
        valid = t["valid"][i]
        if "float" in ty:
            data = np.array([_SPECIAL.get(v, v) if isinstance(v, str) else v for v in vals], dtype=np.float64).astype(npt)
        else:
            data = np.array(vals, dtype=np.float64 if not vals else None).astype(npt)
        out.append(HostColumn(data[:end], None if valid is None else np.array(valid[:end], dtype=bool), ty, offset=off))
    return out


def _nan_rows(c):
    v = np.asarray(c.data)[c.offset:c.offset + c.size]
    if v.dtype.kind != "f":
        return np.zeros(c.size, dtype=bool)
    valid = np.ones(c.size, dtype=bool) if c.valid is None else np.asarray(c.valid[c.offset:c.offset + c.size], dtype=bool)
    return np.isnan(v) & valid


def _groups(cols, nulls_equal, nans_equal):
    """(alone: rows that equal no row, ids: group id of every other row (-1 for the alone ones))."""
    n = cols[0].size
    bits, valid = zip(*[_rows(c) for c in cols])
    alone = np.zeros(n, dtype=bool)
    if not nulls_equal:
        alone |= ~np.logical_and.reduce(valid)
    if not nans_equal:
        alone |= np.logical_or.reduce([_nan_rows(c) for c in cols])
    key = np.stack(list(bits) + [v.astype(np.uint64) for v in valid], axis=1)
    ids = np.full(n, -1, dtype=np.int64)
    if (~alone).any():
        _, inv = np.unique(key[~alone], axis=0, return_inverse=True)
        ids[~alone] = inv.reshape(-1)
    return alone, ids


def distinct_indices(cols, keep, nulls_equal=True, nans_equal=True):
    if not cols or cols[0].size == 0:
        return np.zeros(0, dtype=np.int32)
    n = cols[0].size
    alone, ids = _groups(cols, nulls_equal, nans_equal)
    keep_row = alone.copy()
    rows = np.flatnonzero(~alone)
    g = ids[rows]
    if len(rows):
        ng = g.max() + 1
        first = np.full(ng, n, dtype=np.int64)
        np.minimum.at(first, g, rows)
        last = np.full(ng, -1, dtype=np.int64)
        np.maximum.at(last, g, rows)
        count = np.bincount(g, minlength=ng)
        if keep in ("any", "first"):
            keep_row[first] = True
        elif keep == "last":
            keep_row[last] = True
        elif keep == "none":
            keep_row[first[count == 1]] = True
        else:
            raise ValueError(keep)
    return np.flatnonzero(keep_row).astype(np.int32)


def distinct_count_table(cols, nulls_equal=True):
    if not cols or cols[0].size == 0:
        return 0
    alone, ids = _groups(cols, nulls_equal, True)
    return int(alone.sum()) + (int(ids.max()) + 1 if (~alone).any() else 0)


def distinct_count_column(c, include_nulls, nan_is_null):
    """reference distinct_count.cu:190-219"""
    if c.size == 0:
        return 0
    if c.null_count == c.size:
        return 1 if include_nulls else 0
    count = distinct_count_table([c], True)
    has_null = c.null_count > 0
    if not include_nulls and has_null:
        count -= 1
    if nan_is_null and _nan_rows(c).any() and (has_null or not include_nulls):
        count -= 1
    return count
