"""A numpy restatement of the cudf::distinct_hash_join contract (include/cudf/join/distinct_hash_join.hpp): the checker of the GPU
tests. Columns are oracle.oracle.HostColumn, compared as tests/filtered_join_restatement.py compares them (its _rows).

right_of_left(left, right, nulls_equal) -> int32[nl]: the right row equal to each left row, JoinNoMatch where there is none:
  - rows are compared column by column; NaN equals NaN and -0 equals +0;
  - nulls_equal: a null equals a null in the same column; otherwise a row with a null in any key column matches nothing;
  - no right rows: every entry JoinNoMatch; no left rows: empty.
The right rows are distinct by contract. Where they are not, the FIRST of the equal right rows is named (the library may name
any of them). inner(...) -> (left_idx, right_idx) is derived from it: the left rows that have a match, ascending."""
import json
import os

import numpy as np

from filtered_join_restatement import _rows, host_table  # noqa: F401  (host_table: re-exported for the tests)
from oracle.oracle import TYPE_ID, HostColumn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_distinct_join.json")
JoinNoMatch = -2**31
_NAME_OF_TYPE_ID = {v: k for k, v in TYPE_ID.items()}


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def sequence_table(t):
    """Golden {type, start, step, size} -> one HostColumn holding the arithmetic sequence."""
    from oracle.oracle import NP_OF_TYPE_ID
    npt = NP_OF_TYPE_ID[TYPE_ID[t["type"]]]
    return [HostColumn((t["start"] + t["step"] * np.arange(t["size"], dtype=np.int64)).astype(npt), None, t["type"])]


def case_tables(c):
    """Golden case -> (left, right) HostColumn lists."""
    return tuple(sequence_table(t["sequence"]) if "sequence" in t else host_table(t) for t in (c["left"], c["right"]))


def case_expected(c):
    """Golden case -> {"inner": (left_idx, right_idx)} and / or {"left_join": right_idx}, int32 arrays, as far as the case states."""
    out = {}
    if "inner_sequence" in c:
        out["inner"] = tuple((s["start"] + s["step"] * np.arange(s["size"])).astype(np.int32)
                             for s in (c["inner_sequence"]["left"], c["inner_sequence"]["right"]))
    if "inner" in c:
        out["inner"] = (np.array(c["inner"]["left"], dtype=np.int32), np.array(c["inner"]["right"], dtype=np.int32))
    if "left_join" in c:
        out["left_join"] = np.array(c["left_join"], dtype=np.int32)
    return out


def _row_ids(tables):
    """Equal rows (nulls equal) of the given tables of one schema get equal ids; -> one id array per table."""
    mats = []
    for cols in tables:
        bits, valid = zip(*[_rows(c) for c in cols])
        mats.append(np.stack(list(bits) + [v.astype(np.uint64) for v in valid], axis=1))
    _, ids = np.unique(np.concatenate(mats), axis=0, return_inverse=True)
    ids = ids.reshape(-1)
    out, at = [], 0
    for m in mats:
        out.append(ids[at:at + len(m)])
        at += len(m)
    return out


def _all_valid(cols):
    return np.logical_and.reduce([_rows(c)[1] for c in cols])


def right_of_left(left, right, nulls_equal):
    nl = left[0].size if left else 0
    nr = right[0].size if right else 0
    out = np.full(nl, JoinNoMatch, dtype=np.int32)
    if nl == 0 or nr == 0:
        return out
    assert len(left) == len(right)
    lid, rid = _row_ids([left, right])
    l_ok = np.ones(nl, dtype=bool) if nulls_equal else _all_valid(left)
    r_ok = np.ones(nr, dtype=bool) if nulls_equal else _all_valid(right)
    r_rows = np.flatnonzero(r_ok)
    if len(r_rows) == 0:
        return out
    uniq, first = np.unique(rid[r_rows], return_index=True)  # (the first of equal right rows)
    pos = np.minimum(np.searchsorted(uniq, lid), len(uniq) - 1)
    hit = l_ok & (uniq[pos] == lid)
    out[hit] = r_rows[first[pos[hit]]].astype(np.int32)
    return out


def inner(left, right, nulls_equal):
    r = right_of_left(left, right, nulls_equal)
    hit = r != JoinNoMatch
    return np.flatnonzero(hit).astype(np.int32), r[hit]


def distinct_rows(cols):
    """The first row of every class of equal rows (nulls equal), as new HostColumns without offset: a table that is distinct
    under either null setting."""
    if not cols or cols[0].size == 0:
        return cols
    (ids,) = _row_ids([cols])
    _, first = np.unique(ids, return_index=True)
    keep = np.sort(first)
    out = []
    for c in cols:
        data = np.asarray(c.data)[c.offset:c.offset + c.size][keep]
        valid = None if c.valid is None else np.asarray(c.valid[c.offset:c.offset + c.size], dtype=bool)[keep]
        out.append(HostColumn(data, valid, _NAME_OF_TYPE_ID[c.type_id]))
    return out
