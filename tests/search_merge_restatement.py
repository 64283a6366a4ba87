"""A numpy restatement of the cudf::lower_bound / upper_bound and cudf::merge contracts (include/cudf/search.hpp, merge.hpp): the
checker of the GPU tests. Columns, `orders` and `null_orders` are those of tests/sorting_restatement.py, whose per-column
(flag, code) keys define the comparison.
  - lower_bound / upper_bound(hay_cols, needle_cols, orders, null_orders): the rows of both tables are dense-ranked together by
    their keys (one np.lexsort), then np.searchsorted(left / right) on the ranks.
  - merge_check(inputs, key_cols, orders, null_orders, output): asserts the merge contract, not one order: the output keys are
    sorted, its rows are the inputs' rows as a multiset (bits and validity; a null compares by validity alone), and the rows of each
    input appear in input order. The last needs an INT64 payload column `table_id << 32 | row` (payload_column), named by `id_col`."""
import json
import os

import numpy as np

import sorting_restatement as S
from oracle.oracle import HostColumn

_HERE = os.path.dirname(os.path.abspath(__file__))
_U = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def load_golden(name):
    with open(os.path.join(_HERE, "golden", name)) as f:
        return json.load(f)


def _joint_ranks(hay_cols, needle_cols, orders, null_orders):
    """Dense ranks of the rows of the haystack and of the needles in the order of their union."""
    assert len(hay_cols) == len(needle_cols)
    h = hay_cols[0].size if hay_cols else 0
    n = needle_cols[0].size if needle_cols else 0
    if not hay_cols:
        return np.zeros(h, dtype=np.int64), np.zeros(n, dtype=np.int64)
    orders, null_orders = S._defaults(hay_cols, orders, null_orders)
    keys = []  # most significant first
    for hc, nc, o, no in zip(hay_cols, needle_cols, orders, null_orders):
        assert hc.type_id == nc.type_id
        fh, ch = S._column_keys(hc, o, no)
        fn, cn = S._column_keys(nc, o, no)
        keys += [np.concatenate([fh, fn]), np.concatenate([ch, cn])]
    perm = np.lexsort(keys[::-1])
    step = np.zeros(h + n, dtype=bool)  # the sorted row differs from its predecessor
    for k in keys:
        ks = k[perm]
        step[1:] |= ks[1:] != ks[:-1]
    ranks = np.empty(h + n, dtype=np.int64)
    ranks[perm] = np.cumsum(step)
    return ranks[:h], ranks[h:]


def lower_bound(hay_cols, needle_cols, orders=None, null_orders=None):
    hr, nr = _joint_ranks(hay_cols, needle_cols, orders, null_orders)
    return np.searchsorted(hr, nr, side="left").astype(np.int32)


def upper_bound(hay_cols, needle_cols, orders=None, null_orders=None):
    hr, nr = _joint_ranks(hay_cols, needle_cols, orders, null_orders)
    return np.searchsorted(hr, nr, side="right").astype(np.int32)


# ---------------------------------------------------------------- merge
def payload_column(table_id, n):
    """The INT64 column `table_id << 32 | row` that lets merge_check see where an output row came from."""
    return HostColumn((np.int64(table_id) << np.int64(32)) | np.arange(n, dtype=np.int64))


def _row_records(cols):
    """One tuple per row: (validity, bits or 0 for a null) of every column."""
    per_col = []
    for c in cols:
        v, valid = S._rows(c)
        bits = np.ascontiguousarray(v).view(_U[np.asarray(v).dtype.itemsize]).astype(np.uint64)
        per_col.append((valid, np.where(valid, bits, np.uint64(0))))
    n = cols[0].size if cols else 0
    return [tuple((bool(valid[i]), int(bits[i])) for valid, bits in per_col) for i in range(n)]


def merge_check(inputs, key_cols, orders, null_orders, output, id_col=None):
    """inputs: a list of tables (lists of HostColumns of one schema); output: the merged table, a list of HostColumns."""
    ncols = len(inputs[0])
    assert len(output) == ncols, "the output has another number of columns"
    for c in range(ncols):
        assert output[c].type_id == inputs[0][c].type_id, f"column {c} has another type"
    total = sum(t[0].size for t in inputs)
    assert all(c.size == total for c in output), "the output has another number of rows"
    assert S.is_sorted([output[k] for k in key_cols], orders, null_orders), "the output keys are not sorted"
    want = sorted(r for t in inputs for r in _row_records(t))
    got = _row_records(output)
    assert sorted(got) == want, "the output rows are not the input rows"
    if id_col is not None:
        ids, valid = S._rows(output[id_col])
        assert valid.all()
        ids = np.asarray(ids).astype(np.int64)
        for t in range(len(inputs)):
            rows = ids[(ids >> 32) == t] & 0xFFFFFFFF
            assert np.array_equal(rows, np.arange(inputs[t][0].size)), f"the rows of table {t} are not in input order"


def sort_table(cols, key_cols, orders, null_orders):
    """`cols` with its rows in the stable order of its key columns: a sorted input for merge."""
    idx = S.sorted_order([cols[k] for k in key_cols], orders, null_orders)
    out = []
    for c in cols:
        v, valid = S._rows(c)
        out.append(HostColumn(np.asarray(v)[idx].astype(np.asarray(c.data).dtype), None if c.valid is None else valid[idx],
                              _type_name(c)))
    return out


def _type_name(c):
    from oracle.oracle import TYPE_ID
    return next(k for k, v in TYPE_ID.items() if v == c.type_id)


# ---------------------------------------------------------------- the golden vectors
def golden_table(t, ty):
    return S.golden_table(t, ty)


def golden_types(c):
    return S.golden_types(c)
