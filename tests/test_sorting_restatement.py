"""CPU: the numpy restatement of cudf::sorted_order / is_sorted (tests/sorting_restatement.py) against the golden vectors
(tests/golden/kat_sorting.json) and against Python's sorted() on tuples, and its packed words against the order they must give."""
import math

import numpy as np
import pytest

import sorting_restatement as R
from oracle.oracle import NP_OF_TYPE_ID, TYPE_ID, HostColumn

GOLD = R.load_golden()
CASES = [(kind, c, ty) for kind in ("sort", "stable_sort") for c in GOLD[kind] for ty in R.golden_types(c)]


def _gathered(cols, idx):
    out = []
    for c in cols:
        v, valid = R._rows(c)
        code, _ = R.value_code(c)
        out.append((np.where(valid, code, 0)[idx].tolist(), valid[idx].tolist()))
    return out


@pytest.mark.parametrize("kind,c,ty", CASES, ids=lambda x: x["name"] if isinstance(x, dict) else x)
def test_golden_orders(kind, c, ty):
    cols = R.golden_table(c["input"], ty)
    got = R.sorted_order(cols, c["orders"], c["null_orders"])
    expect = np.array(R.golden_expect(c, ty), dtype=np.int32)
    if c.get("compare") == "gathered":
        assert _gathered(cols, got) == _gathered(cols, expect)
    else:
        assert got.tolist() == expect.tolist()
    assert R.is_sorted([HostColumn(np.asarray(k.data)[k.offset:][got], None if k.valid is None else k.valid[k.offset:][got],
                                   [n for n, i in TYPE_ID.items() if i == k.type_id][0]) for k in cols], c["orders"], c["null_orders"])


@pytest.mark.parametrize("c", GOLD["is_sorted"], ids=lambda c: c["name"])
def test_golden_is_sorted(c):
    for ty in R.NUMERIC_CHRONO:
        assert R.is_sorted(R.is_sorted_columns(GOLD, c, ty), c["orders"], c["null_orders"]) == c["expect"], ty


TYPES = ["int8", "int16", "int32", "int64", "uint32", "uint64", "float32", "float64", "bool", "decimal64"]
FLOAT_POOL = [0.0, -0.0, math.inf, -math.inf, math.nan, -1.5, 2.25, 1e30]


def random_table(rng, n, ncols):
    cols, orders, null_orders = [], [], []
    for _ in range(ncols):
        ty = TYPES[rng.integers(len(TYPES))]
        npt = np.dtype(NP_OF_TYPE_ID[TYPE_ID[ty]])
        if npt.kind == "f":
            data = np.array(FLOAT_POOL, dtype=npt)[rng.integers(0, len(FLOAT_POOL), n)]
        elif npt.kind == "b":
            data = rng.random(n) < 0.5
        else:
            data = rng.integers(-3 if npt.kind == "i" else 0, 4, n).astype(npt)
        valid = rng.random(n) < 0.7 if rng.random() < 0.4 else None
        cols.append(HostColumn(data, valid, ty))
        orders.append("desc" if rng.random() < 0.5 else "asc")
        null_orders.append("after" if rng.random() < 0.5 else "before")
    return cols, orders, null_orders


def _tuple_key(cols, orders, null_orders, i):
    """Row i as a tuple Python compares the way the contract does."""
    key = []
    for c, o, no in zip(cols, orders, null_orders):
        v, valid = R._rows(c)
        x = v[i]
        if v.dtype.kind == "f":
            rank = (2, 0.0) if math.isnan(x) else (1, float(x) + 0.0)  # NaN above +inf; -0 == +0
        else:
            rank = (1, int(x))
        sign = -1 if o == "desc" else 1
        val = (sign * rank[0], sign * rank[1])
        if valid[i]:
            key.append((1, val) if (no == "before") != (o == "desc") else (0, val))
        else:
            key.append((0, (0, 0)) if (no == "before") != (o == "desc") else (1, (0, 0)))
    return tuple(key)


@pytest.mark.parametrize("seed", range(40))
def test_random_against_python_sorted(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(0, 40))
    cols, orders, null_orders = random_table(rng, n, int(rng.integers(1, 5)))
    keys = [_tuple_key(cols, orders, null_orders, i) for i in range(n)]
    expect = sorted(range(n), key=lambda i: keys[i])  # (sorted is stable)
    assert R.sorted_order(cols, orders, null_orders).tolist() == expect
    assert R.is_sorted(cols, orders, null_orders) == all(keys[i] <= keys[i + 1] for i in range(n - 1))
    # the packed words give the same order: sorting by the words, least significant first, with a stable sort
    order = np.arange(n)
    for w in R.packed_words(cols, orders, null_orders):
        order = order[np.argsort(w[order], kind="stable")]
    assert order.tolist() == expect


def test_packed_word_shapes():
    """The word counts and pass counts the layout promises ("Sorting")."""
    rng = np.random.default_rng(0)
    n = 8192
    i32 = lambda: HostColumn(rng.integers(-2**31, 2**31, n).astype(np.int32))
    some = rng.random(n) < 0.9
    w = R.packed_words([i32(), i32()])
    assert len(w) == 1 and R.expected_passes(w) == 8
    assert len(R.packed_words([i32(), HostColumn(rng.integers(-2**31, 2**31, n).astype(np.int32), some)])) == 2  # 65 bits
    w = R.packed_words([HostColumn(rng.integers(-2**63, 2**63, n).astype(np.int64), some)])
    assert len(w) == 2 and R.expected_passes(w[1:]) == 1  # the second word is the null bit
    w = R.packed_words([HostColumn(rng.random(n) < 0.5), HostColumn(rng.integers(-128, 128, n).astype(np.int8)),
                        HostColumn(rng.integers(-2**15, 2**15, n).astype(np.int16), some)], ["asc", "asc", "desc"])
    assert len(w) == 1 and R.expected_passes(w) <= 4  # 26 bits
    assert len(R.packed_words([HostColumn(rng.integers(-128, 128, n).astype(np.int8)) for _ in range(16)])) == 2
    assert R.expected_passes(R.packed_words([HostColumn(np.full(n, 7, dtype=np.int64))])) == 0
    assert R.expected_passes(R.packed_words([HostColumn(rng.integers(0, 200, n).astype(np.int32))])) == 1
