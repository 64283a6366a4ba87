"""A numpy restatement of the cudf::sorted_order / is_sorted contract (include/cudf/sorting.hpp) and of the packed radix words
the library sorts by (cudf_amd/csrc/sorting/sorting_impl.hpp): the checker of the GPU tests.

A column is a HostColumn (values, valid, offset). `orders` / `null_orders` are lists of "asc" / "desc" and "before" / "after"
(empty: all "asc" / all "before").
  - sorted_order(cols, orders, null_orders): the stable permutation, by np.lexsort over per-column (null flag, code) keys.
  - is_sorted(cols, orders, null_orders): no row is lexicographically less than its predecessor.
  - packed_words(cols, orders, null_orders): the uint64 word arrays, least significant word first; expected_passes(words): the
    radix passes they cost, the number of bytes in which the OR and the AND of a word's values differ, summed over the words.
Within a column: -0 == +0, every NaN is one value above +inf, bool compares as 0 / 1; "before": a null is smaller than every value;
"desc" flips the whole comparison of the column, nulls included."""
import json
import os

import numpy as np

from oracle.oracle import NP_OF_TYPE_ID, TYPE_ID, HostColumn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_sorting.json")
_SPECIAL = {"nan": np.nan, "-nan": -np.nan, "inf": np.inf, "-inf": -np.inf}
_U = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def type_class(ty):
    """"bool", "unsigned", "float" or "signed" (timestamps, durations and decimals are signed integers)."""
    if ty == "bool":
        return "bool"
    return "unsigned" if ty.startswith("uint") else "float" if ty.startswith("float") else "signed"


def host_column(ty, vals, valid=None, offset=0):
    """Golden values -> HostColumn of type `ty`. Integers wrap into the type (as the reference's typed tests construct T(-2));
    bool is value != 0; "lowest" / "max" are the type's limits; floats take "nan", "-nan", "inf", "-inf"."""
    npt = np.dtype(NP_OF_TYPE_ID[TYPE_ID[ty]])
    if npt.kind == "f":
        lim = {"lowest": float(np.finfo(npt).min), "max": float(np.finfo(npt).max)}
        data = np.array([_SPECIAL.get(v, lim.get(v, v)) if isinstance(v, str) else v for v in vals], dtype=np.float64).astype(npt)
        bits = data.view(_U[npt.itemsize])
        for j, v in enumerate(vals):  # (numpy drops the sign of -nan on the way: set it on the bits)
            if v == "-nan":
                bits[j] |= bits.dtype.type(1) << bits.dtype.type(8 * npt.itemsize - 1)
    elif npt.kind == "b":
        data = np.array([v != 0 and v != "lowest" for v in vals], dtype=np.bool_)
    else:
        lim = {"lowest": int(np.iinfo(npt).min), "max": int(np.iinfo(npt).max)}
        span = 1 << (8 * npt.itemsize)
        ints = [lim[v] if isinstance(v, str) else int(v) for v in vals]
        data = np.array([(v % span) - (span if npt.kind == "i" and (v % span) >= span // 2 else 0) for v in ints], dtype=npt)
    return HostColumn(data, None if valid is None else np.array(valid, dtype=bool), ty, offset=offset)


def _rows(c):
    v = np.asarray(c.data)[c.offset:c.offset + c.size]
    valid = np.ones(c.size, dtype=bool) if c.valid is None else np.asarray(c.valid[c.offset:c.offset + c.size], dtype=bool)
    return v, valid


def value_code(c):
    """(code, vbits): the width-tight order-preserving code of every row (unsigned comparison == ascending order of values)."""
    v, _ = _rows(c)
    npt = np.dtype(NP_OF_TYPE_ID[c.type_id])
    w = npt.itemsize
    if npt.kind == "b":
        return (v != 0).astype(np.uint64), 1
    if npt.kind == "f":
        f = v.astype(npt, copy=True)
        f[f == 0] = 0.0  # -0 -> +0
        bits = f.view(_U[w]).astype(np.uint64)
        bits[np.isnan(f)] = 0x7FC00000 if w == 4 else 0x7FF8000000000000  # one NaN, above +inf
        sign = np.uint64(1) << np.uint64(8 * w - 1)
        full = np.uint64((1 << (8 * w)) - 1)
        return np.where(bits & sign != 0, bits ^ full, bits ^ sign).astype(np.uint64), 8 * w
    bits = v.astype(npt).view(_U[w]).astype(np.uint64)
    if npt.kind == "i":
        bits = bits ^ (np.uint64(1) << np.uint64(8 * w - 1))
    return bits, 8 * w


def _defaults(cols, orders, null_orders):
    orders = list(orders) if orders else ["asc"] * len(cols)
    null_orders = list(null_orders) if null_orders else ["before"] * len(cols)
    assert len(orders) == len(cols) and len(null_orders) == len(cols)
    return orders, null_orders


def _column_keys(c, order, null_order):
    """(flag, code) of a column: rows compare by flag first, then by code; the flag is 0 for the kind of row that comes first."""
    code, vbits = value_code(c)
    _, valid = _rows(c)
    if order == "desc":
        code = ~code & np.uint64((1 << vbits) - 1)
    code = np.where(valid, code, np.uint64(0))
    nulls_first = (null_order == "before") != (order == "desc")
    flag = (valid == nulls_first).astype(np.uint64)
    return flag, code


def sorted_order(cols, orders=None, null_orders=None):
    if not cols:
        return np.zeros(0, dtype=np.int32)
    orders, null_orders = _defaults(cols, orders, null_orders)
    keys = []  # most significant first
    for c, o, no in zip(cols, orders, null_orders):
        keys += list(_column_keys(c, o, no))
    return np.lexsort(keys[::-1]).astype(np.int32)  # (lexsort: the last key is the primary one; it is stable)


def is_sorted(cols, orders=None, null_orders=None):
    if not cols or cols[0].size <= 1:
        return True
    orders, null_orders = _defaults(cols, orders, null_orders)
    n = cols[0].size
    decided = np.zeros(n - 1, dtype=bool)
    less = np.zeros(n - 1, dtype=bool)  # row i + 1 < row i
    for c, o, no in zip(cols, orders, null_orders):
        for k in _column_keys(c, o, no):
            lt, gt = k[1:] < k[:-1], k[1:] > k[:-1]
            less |= ~decided & lt
            decided |= lt | gt
    return not less.any()


def packed_words(cols, orders=None, null_orders=None):
    """The words of sorting_impl.hpp: fields placed from the last column up, a new word when a field does not fit, the 64 value
    bits of a nullable 8-byte column in a word of their own and its null bit lowest in the next."""
    if not cols:
        return []
    orders, null_orders = _defaults(cols, orders, null_orders)
    n = cols[0].size
    words, cur, used = [], np.zeros(n, dtype=np.uint64), 0

    def close():
        nonlocal cur, used
        if used:
            words.append(cur)
        cur, used = np.zeros(n, dtype=np.uint64), 0
    for c, o, no in list(zip(cols, orders, null_orders))[::-1]:
        flag, code = _column_keys(c, o, no)
        _, vbits = value_code(c)
        nbit = 1 if c.null_count > 0 else 0
        if vbits + nbit > 64:
            close()
            words.append(code)
            cur, used = flag.copy(), 1
            continue
        if used + vbits + nbit > 64:
            close()
        cur = cur | (code << np.uint64(used))
        if nbit:
            cur = cur | (flag << np.uint64(used + vbits))
        used += vbits + nbit
    close()
    return words


def expected_passes(words):
    total = 0
    for w in words:
        if len(w) == 0:
            continue
        differ = int(np.bitwise_or.reduce(w)) ^ int(np.bitwise_and.reduce(w))
        total += sum(1 for b in range(8) if (differ >> (8 * b)) & 0xFF)
    return total


# ---------------------------------------------------------------- the golden vectors
def golden_table(t, ty):
    """A golden table instantiated for type `ty`: columns of type "T" take `ty`, the others are as written."""
    cols = []
    for i, (cty, vals) in enumerate(zip(t["types"], t["cols"])):
        valid = t["valid"][i] if "valid" in t else None
        off = t.get("offset", [0] * len(t["cols"]))[i]
        cols.append(host_column(ty if cty == "T" else cty, vals, valid, off))
    return cols


def golden_expect(c, ty):
    """The expected order of case `c` for type `ty`: expect_bool / expect_unsigned where the reference's test carries one."""
    return c.get("expect_" + type_class(ty), c["expect"])


NUMERIC_CHRONO = [t for t in TYPE_ID if not t.startswith("decimal")]


def golden_types(c):
    """The types case `c` is instantiated for."""
    return NUMERIC_CHRONO if c["for"] == "numeric_chrono" else c["for"]


def is_sorted_columns(gold, c, ty):
    """The columns of an is_sorted case for type `ty`, from the golden file's is_sorted_data."""
    cls = "chrono" if ty.startswith(("timestamp", "duration")) else type_class(ty)
    cls = "signed" if cls == "float" else cls
    cols = []
    for name in c["columns"]:
        d = gold["is_sorted_data"][name]
        cols.append(host_column(ty, d.get(cls, d.get("all")), d.get("valid")))
    return cols
