"""CPU tests of the checker the GPU tests of cudf::lower_bound / upper_bound / merge rely on (tests/search_merge_restatement.py): the
golden vectors (tests/golden/kat_search.json, kat_merge.json), the bounds against a brute-force comparison of Python tuples on
seeded random small tables, and merge_check against one correct and three hand-made wrong merges."""
import functools

import numpy as np
import pytest

import search_merge_restatement as R
import sorting_restatement as S
from oracle.oracle import HostColumn

SEARCH = R.load_golden("kat_search.json")
MERGE = R.load_golden("kat_merge.json")
TYPES = ["int8", "int16", "int32", "int64", "uint8", "uint32", "uint64", "float32", "float64", "bool", "decimal32", "timestamp_ms"]
FLOAT_POOL = [0.0, -0.0, np.inf, -np.inf, np.nan, -1.5, 2.25, 1e30, -3e-5]


def search_types(c):
    return ["int64"] if c["for"] == ["as_written"] else c["for"]


def merge_tables(c, ty):
    tables = [S.golden_table(t, ty) for t in c["tables"]]
    return tables * c.get("copies", 1)


@pytest.mark.parametrize("c", SEARCH["cases"], ids=lambda c: c["name"])
def test_golden_search(c):
    fn = R.lower_bound if c["fn"] == "lower" else R.upper_bound
    for ty in search_types(c):
        got = fn(S.golden_table(c["haystack"], ty), S.golden_table(c["needles"], ty), c["orders"], c["null_orders"])
        assert got.dtype == np.int32 and got.tolist() == c["expect"], ty


def _same_table(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        (gv, gm), (wv, wm) = S._rows(g), S._rows(w)
        assert g.type_id == w.type_id and np.array_equal(gm, wm)
        assert np.array_equal(np.asarray(gv)[gm], np.asarray(wv)[wm])


@pytest.mark.parametrize("c", MERGE["cases"], ids=lambda c: c["name"])
def test_golden_merge(c):
    """The reference's expected table passes merge_check and is the stable sort of the concatenation."""
    for ty in c["for"][:3] + c["for"][-1:]:
        tables = merge_tables(c, ty)
        expect = S.golden_table(c["expect"], ty)
        R.merge_check(tables, c["key_cols"], c["orders"], c["null_orders"], expect)
        _same_table(R.sort_table(_concat(tables), c["key_cols"], c["orders"], c["null_orders"]), expect)


def _concat(tables):
    out = []
    for c in range(len(tables[0])):
        rows = [S._rows(t[c]) for t in tables]
        any_valid = any(t[c].valid is not None for t in tables)
        out.append(HostColumn(np.concatenate([np.asarray(v) for v, _ in rows]),
                              np.concatenate([m for _, m in rows]) if any_valid else None, R._type_name(tables[0][c])))
    return out


def test_golden_generated_and_errors_are_well_formed():
    g = MERGE["generated"][0]
    assert g["name"] == "KeysWithNulls" and g["rows"] == 13200 and g["nulls_at_multiples_of"] == [10, 15]
    assert len(MERGE["errors"]) >= 7 and all(e["raises"] == "logic_error" for e in MERGE["errors"])


# ---------------------------------------------------------------- the bounds against brute force
def _rand_col(rng, ty, n, nullable, universe=4):
    from oracle.oracle import NP_OF_TYPE_ID, TYPE_ID
    npt = np.dtype(NP_OF_TYPE_ID[TYPE_ID[ty]])
    if npt.kind == "b":
        data = rng.random(n) < 0.5
    elif npt.kind == "f":
        data = np.array(FLOAT_POOL, dtype=npt)[rng.integers(0, len(FLOAT_POOL), n)]
    else:
        lo = -(universe // 2) if npt.kind == "i" else 0
        data = rng.integers(lo, lo + universe, n).astype(npt)
    return HostColumn(data, rng.random(n) < 0.7 if nullable else None, ty)


def _py_key(col, order, null_order):
    """One comparable Python value per row: (class, value) with the class placing nulls and NaN."""
    v, valid = S._rows(col)
    out = []
    for x, ok in zip(np.asarray(v).tolist(), valid.tolist()):
        if not ok:
            k = (0, 0) if null_order == "before" else (3, 0)
        elif isinstance(x, float) and x != x:
            k = (2, 0)
        else:
            k = (1, (1 if x else 0) if col.type_id == 11 else x + 0.0 if isinstance(x, float) else x)
        out.append(k)
    return out, order == "desc"


def _less(a, b, descs):
    for x, y, d in zip(a, b, descs):
        if x != y:
            return (x > y) if d else (x < y)
    return False


@functools.lru_cache(maxsize=None)
def _brute_case(seed):
    rng = np.random.default_rng(seed)
    ncols = int(rng.integers(1, 4))
    types = [TYPES[rng.integers(len(TYPES))] for _ in range(ncols)]
    h, n = int(rng.integers(0, 24)), int(rng.integers(0, 12))
    sides = [rng.random() < 0.5, rng.random() < 0.5]  # nulls on the haystack / on the needles
    orders = ["desc" if rng.random() < 0.5 else "asc" for _ in types]
    null_orders = ["after" if rng.random() < 0.5 else "before" for _ in types]
    hay = R.sort_table([_rand_col(rng, t, h, sides[0]) for t in types], list(range(ncols)), orders, null_orders)
    needles = [_rand_col(rng, t, n, sides[1]) for t in types]
    return hay, needles, orders, null_orders


@pytest.mark.parametrize("seed", range(200))
def test_bounds_against_brute_force(seed):
    hay, needles, orders, null_orders = _brute_case(seed)
    hk = [_py_key(c, o, no) for c, o, no in zip(hay, orders, null_orders)]
    nk = [_py_key(c, o, no) for c, o, no in zip(needles, orders, null_orders)]
    descs = [d for _, d in hk]
    hrows = list(zip(*[k for k, _ in hk])) if hay[0].size else []
    nrows = list(zip(*[k for k, _ in nk])) if needles[0].size else []
    lower = [sum(_less(r, x, descs) for r in hrows) for x in nrows]
    upper = [sum(not _less(x, r, descs) for r in hrows) for x in nrows]
    assert R.lower_bound(hay, needles, orders, null_orders).tolist() == lower
    assert R.upper_bound(hay, needles, orders, null_orders).tolist() == upper


# ---------------------------------------------------------------- merge_check
def _two_tables():
    a = [HostColumn(np.array([1, 1, 2, 5], dtype=np.int32), np.array([1, 1, 1, 0], dtype=bool)), R.payload_column(0, 4)]
    b = [HostColumn(np.array([1, 2, 2], dtype=np.int32)), R.payload_column(1, 3)]
    p = lambda t, r: (t << 32) | r
    good = [HostColumn(np.array([1, 1, 1, 2, 2, 2, 9], dtype=np.int32), np.array([1, 1, 1, 1, 1, 1, 0], dtype=bool)),
            HostColumn(np.array([p(0, 0), p(1, 0), p(0, 1), p(1, 1), p(0, 2), p(1, 2), p(0, 3)], dtype=np.int64))]
    return [a, b], good


def _edit(table, rows):
    return [HostColumn(np.asarray(c.data)[rows], None if c.valid is None else c.valid[rows], R._type_name(c)) for c in table]


def test_merge_check_accepts_and_rejects():
    inputs, good = _two_tables()
    args = ([0], ["asc"], ["after"])
    R.merge_check(inputs, *args, good, id_col=1)  # (the null's value differs from the input's: only its validity counts)
    with pytest.raises(AssertionError):  # a row dropped
        R.merge_check(inputs, *args, _edit(good, [0, 1, 2, 3, 4, 6]), id_col=1)
    with pytest.raises(AssertionError, match="input order"):  # two equal-key rows of table 0 swapped
        R.merge_check(inputs, *args, _edit(good, [2, 1, 0, 3, 4, 5, 6]), id_col=1)
    with pytest.raises(AssertionError, match="not sorted"):  # a row out of order
        R.merge_check(inputs, *args, _edit(good, [0, 1, 3, 2, 4, 5, 6]), id_col=1)
    with pytest.raises(AssertionError, match="not the input rows"):  # a row replaced by a copy of another
        R.merge_check(inputs, *args, _edit(good, [0, 1, 1, 3, 4, 5, 6]), id_col=1)
