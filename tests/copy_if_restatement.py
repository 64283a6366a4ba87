"""A numpy restatement of cudf::apply_boolean_mask, apply_deletion_mask, drop_nulls, drop_nans, unique
(include/cudf/stream_compaction.hpp) and cudf::unique_count (include/cudf/reduction/unique_count.hpp), rule for rule as the
headers state the contract: the checker of the GPU tests.

A column is a HostColumn (values, valid, offset). Every table function returns the ascending int64 indices of the surviving rows;
rows stay whole, so the expected table is take(cols, idx). The rejected inputs raise LogicError (cudf::logic_error) or IndexError
(std::out_of_range)."""
import json
import os

import numpy as np

from filtered_join_restatement import _SPECIAL, _rows
from filtered_join_restatement import host_table as _host_table
from oracle.oracle import TYPE_ID

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_KEY_COLUMNS = 16


class LogicError(Exception):
    pass


def load_golden():
    """{"stream_compaction": kat_stream_compaction.json, "unique_count": kat_unique_count.json}"""
    out = {}
    for k in ("stream_compaction", "unique_count"):
        with open(os.path.join(GOLDEN_DIR, f"kat_{k}.json")) as f:
            out[k] = json.load(f)
    return out


def host_table(t):
    """Golden table {types, cols, valid, [offset], [scale]} -> list of HostColumn."""
    cols = _host_table(t)
    for c, s in zip(cols, t.get("scale", [0] * len(cols))):
        c.scale = s
    return cols


def values(c):
    return np.asarray(c.data)[c.offset:c.offset + c.size]


def valid(c):
    return np.ones(c.size, dtype=bool) if c.valid is None else np.asarray(c.valid[c.offset:c.offset + c.size], dtype=bool)


def take(cols, idx):
    """The rows idx of every column: [(values, valid or None when the column has no mask)]."""
    return [(values(c)[idx], None if c.valid is None else valid(c)[idx]) for c in cols]


def _nrows(cols):
    return cols[0].size if cols else 0


def _none():
    return np.zeros(0, dtype=np.int64)


def _select(cols, keys):
    for k in keys:
        if not 0 <= k < len(cols):
            raise IndexError(k)
    return [cols[k] for k in keys]


def _key_limits(keys):
    if len(keys) > MAX_KEY_COLUMNS:
        raise LogicError("more than 16 key columns")


def _is_nan(c):
    v = values(c)
    return np.isnan(v) if v.dtype.kind == "f" else np.zeros(c.size, dtype=bool)


# ---------------------------------------------------------------- the masks
def apply_boolean_mask(cols, mask, deletion=False):
    n = _nrows(cols)
    if mask.size == 0:  # (first, as the reference: an empty table whatever the input's size)
        return _none()
    if mask.type_id != TYPE_ID["bool"]:
        raise LogicError("Mask must be Boolean type")
    if n != 0 and n != mask.size:
        raise LogicError("Column size mismatch")
    if n == 0:
        return _none()
    v = values(mask) != 0
    keep = valid(mask) & (~v if deletion else v)  # deletion: valid and false; a null element deletes the row
    return np.flatnonzero(keep).astype(np.int64)


def apply_deletion_mask(cols, mask):
    return apply_boolean_mask(cols, mask, deletion=True)


# ---------------------------------------------------------------- drop_nulls / drop_nans
def drop_nulls(cols, keys, keep_threshold=None):
    kc = _select(cols, keys)
    n = _nrows(cols)
    thr = len(keys) if keep_threshold is None else keep_threshold
    if not kc or n == 0 or not any(c.null_count > 0 for c in kc):
        return np.arange(n, dtype=np.int64)  # a copy, whatever the threshold
    _key_limits(kc)
    count = np.sum([valid(c) for c in kc], axis=0)  # a key without a mask is valid in every row
    return np.flatnonzero(count >= thr).astype(np.int64)


def drop_nans(cols, keys, keep_threshold=None):
    kc = _select(cols, keys)
    n = _nrows(cols)
    thr = len(keys) if keep_threshold is None else keep_threshold
    if not kc or n == 0:
        return np.arange(n, dtype=np.int64)
    if any(c.type_id not in (TYPE_ID["float32"], TYPE_ID["float64"]) for c in kc):
        raise LogicError("Key column is not of type floating-point")
    _key_limits(kc)
    count = np.sum([~valid(c) | ~_is_nan(c) for c in kc], axis=0)  # a null field counts as not NaN
    return np.flatnonzero(count >= thr).astype(np.int64)


# ---------------------------------------------------------------- unique / unique_count
def _equals_previous(kc, nulls_equal):
    """eq[i]: row i equals row i - 1 (eq[0] is False): NaN == NaN, -0 == +0, nulls by nulls_equal."""
    n = kc[0].size
    eq = np.ones(n, dtype=bool)
    eq[0] = False
    for c in kc:
        bits, m = _rows(c)
        both = m[1:] & m[:-1]
        neither = ~m[1:] & ~m[:-1]
        eq[1:] &= (both & (bits[1:] == bits[:-1])) | (neither if nulls_equal else False)
    return eq


def unique(cols, keys, keep, nulls_equal=True):
    n = _nrows(cols)
    if n == 0 or not cols or not keys:
        return _none()  # (before the keys are looked at)
    kc = _select(cols, keys)
    _key_limits(kc)
    eq = _equals_previous(kc, nulls_equal)
    first = ~eq  # i == 0 or row i differs from row i - 1
    last = np.append(~eq[1:], True)  # i == n - 1 or row i differs from row i + 1
    sel = {"any": first, "first": first, "last": last, "none": first & last}[keep]
    return np.flatnonzero(sel).astype(np.int64)


def unique_count_table(cols, nulls_equal=True):
    if _nrows(cols) == 0:
        return 0
    _key_limits(cols)
    return int((~_equals_previous(cols, nulls_equal)).sum())


def unique_count_column(c, include_nulls, nan_is_null):
    if c.size == 0 or c.null_count == c.size:
        return 0
    null = ~valid(c)
    nan = _is_nan(c) if nan_is_null else np.zeros(c.size, dtype=bool)
    eq = _equals_previous([c], True)
    count = 0
    for i in range(c.size):
        if not include_nulls and (null[i] or nan[i]):  # 1.
            continue
        if i == 0:  # 2.
            count += 1
        elif include_nulls and nan_is_null and (null[i] or nan[i]):  # 3.
            count += not (null[i - 1] or _is_nan(c)[i - 1])
        else:  # 4.
            count += not eq[i]
    return count


# ---------------------------------------------------------------- the golden vectors' call shapes and comparison
def check_expected(got, expect):
    """got: [(values, valid or None)]; expect: golden {cols, valid}. Values under a null are not compared; an expected column of
    zero rows says nothing about a mask."""
    assert len(got) == len(expect["cols"])
    for (gv, gm), ev, em in zip(got, expect["cols"], expect["valid"]):
        assert len(gv) == len(ev)
        if len(ev) == 0:
            continue
        assert (gm is None) == (em is None)
        m = np.ones(len(ev), dtype=bool) if em is None else np.array(em, dtype=bool)
        if gm is not None:
            assert np.array_equal(np.asarray(gm, dtype=bool), m)
        e = np.array([_SPECIAL.get(x, x) if isinstance(x, str) else x for x in ev], dtype=np.float64)
        g = np.asarray(gv).astype(np.float64)
        assert np.array_equal(g[m], e[m], equal_nan=True)


def run_case(kind, c, fns):
    """Runs golden case c of `kind` through fns (the restatement's call shapes) -> surviving rows, or the exception it pins."""
    cols = host_table(c["input"])
    if kind in ("apply_boolean_mask", "apply_deletion_mask"):
        call = lambda: fns[kind](cols, host_table(c["mask"])[0])
    elif kind in ("drop_nulls", "drop_nans"):
        call = lambda: fns[kind](cols, c["keys"], c.get("threshold"))
    else:
        call = lambda: fns[kind](cols, c["keys"], c["keep"], c["nulls"] == "equal")
    return cols, call
