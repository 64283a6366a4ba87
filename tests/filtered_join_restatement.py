"""A numpy restatement of the cudf::filtered_join contract (include/cudf/join/filtered_join.hpp): the checker of the GPU tests.

A column is (values, valid, offset) as oracle.oracle.HostColumn holds it. semi_anti(left, right, nulls_equal) -> (semi, anti), the
ascending int32 left row indices that have / have no equal row in `right`:
  - rows are compared column by column; NaN equals NaN and -0 equals +0 (floats compare by their normalised bits);
  - nulls_equal: a null equals a null in the same column; otherwise a row with a null in any key column matches nothing;
  - no left rows: both empty; no right rows: semi empty, anti every left row."""
import json
import os

import numpy as np

from oracle.oracle import NP_OF_TYPE_ID, TYPE_ID, HostColumn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_semi_anti_join.json")
_SPECIAL = {"nan": np.nan, "-nan": -np.nan, "inf": np.inf, "-inf": -np.inf}


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def host_table(t):
    """Golden table {types, cols, valid, [offset]} -> list of HostColumn (the column's rows start at `offset` of its buffer)."""
    out = []
    for i, (ty, vals) in enumerate(zip(t["types"], t["cols"])):
        npt = NP_OF_TYPE_ID[TYPE_ID[ty]]
        off = t.get("offset", [0] * len(t["cols"]))[i]
        valid = t["valid"][i]
        if "float" in ty:
            data = np.array([_SPECIAL.get(v, v) if isinstance(v, str) else v for v in vals], dtype=np.float64).astype(npt)
            if any(v == "-nan" for v in vals):  # (numpy drops the sign of -nan on the way: set it on the bits)
                bits = data.view(np.uint32 if npt == np.float32 else np.uint64)
                sign = np.uint32(1 << 31) if npt == np.float32 else np.uint64(1 << 63)
                for j, v in enumerate(vals):
                    if v == "-nan":
                        bits[j] |= sign
        else:
            data = np.array(vals, dtype=npt)
        out.append(HostColumn(data, None if valid is None else np.array(valid, dtype=bool), ty, offset=off))
    return out


def _rows(c):
    """HostColumn -> (normalised key bits as uint64, validity) of its rows."""
    v = np.asarray(c.data)[c.offset:c.offset + c.size]
    valid = np.ones(c.size, dtype=bool) if c.valid is None else np.asarray(c.valid[c.offset:c.offset + c.size], dtype=bool)
    if v.dtype.kind == "f":
        v = v.astype(np.float64)
        v = np.where(v == 0, 0.0, v)  # -0 -> +0
        bits = v.view(np.uint64).copy()
        bits[np.isnan(v)] = np.uint64(0x7FF8000000000000)  # one NaN
    elif v.dtype.kind == "b" or c.type_id == TYPE_ID["bool"]:
        bits = (v != 0).astype(np.uint64)
    else:
        bits = v.astype(np.int64).view(np.uint64) if v.dtype.kind == "i" else v.astype(np.uint64)
    return np.where(valid, bits, np.uint64(0)), valid


def semi_anti(left, right, nulls_equal):
    nl = left[0].size if left else 0
    nr = right[0].size if right else 0
    none = np.zeros(0, dtype=np.int32)
    if nl == 0:
        return none, none
    if nr == 0:
        return none, np.arange(nl, dtype=np.int32)
    assert len(left) == len(right)
    lb, lv = zip(*[_rows(c) for c in left])
    rb, rv = zip(*[_rows(c) for c in right])
    # one row of the key = every column's bits and validity; equal rows get equal ids
    L = np.stack(list(lb) + [x.astype(np.uint64) for x in lv], axis=1)
    R = np.stack(list(rb) + [x.astype(np.uint64) for x in rv], axis=1)
    _, ids = np.unique(np.concatenate([L, R]), axis=0, return_inverse=True)
    ids = ids.reshape(-1)
    lid, rid = ids[:nl], ids[nl:]
    l_ok = np.ones(nl, dtype=bool) if nulls_equal else np.logical_and.reduce(lv)
    r_ok = np.ones(nr, dtype=bool) if nulls_equal else np.logical_and.reduce(rv)
    hit = l_ok & np.isin(lid, rid[r_ok])
    return np.flatnonzero(hit).astype(np.int32), np.flatnonzero(~hit).astype(np.int32)
