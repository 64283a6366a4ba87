"""GPU tests of cudf::sorted_order, sort, sort_by_key, their stable forms and is_sorted through the C ABI and cudf_amd.sorting: the
golden vectors (tests/golden/kat_sorting.json) over every numeric, timestamp and duration type, seeded random tables against the
numpy restatement (tests/sorting_restatement.py) at the wave and tile edges of the radix sort, the shapes of the packed-word plan
proven by the kernels that ran, sliced and payload columns, a second stream, the rejected inputs, is_sorted at its edges and a
16M-row property against torch."""
import functools

import numpy as np
import pytest

import sorting_restatement as R

pytestmark = pytest.mark.gpu

GOLD = R.load_golden()
ORDER_CASES = [(kind, c, ty) for kind in ("sort", "stable_sort") for c in GOLD[kind] for ty in R.golden_types(c)]
ROWS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 12289]  # the wave (64) and radix tile (4096) edges
TYPES = ["int8", "int16", "int32", "int64", "uint32", "uint64", "float32", "float64", "bool", "decimal64"]


@pytest.fixture(scope="module")
def G(gpu):
    import gpu_backend
    return gpu_backend


def _table(G, cols):
    import cudf_amd
    return cudf_amd.Table([G.to_device(c) for c in cols])


def _enums(orders, null_orders):
    from cudf_amd.types import NullOrder, Order
    return ([Order.DESCENDING if o == "desc" else Order.ASCENDING for o in orders],
            [NullOrder.BEFORE if o == "before" else NullOrder.AFTER for o in null_orders])


def _indices(col, n):
    assert col.type().id().name == "INT32" and col.null_count() == 0 and col.size() == n
    return np.asarray(col.to_numpy()[0])


def _kernels_of(fn):
    from cudf_amd import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
    finally:
        _lib.profile_enable(False)
    return out, {k: v[0] for k, v in _lib.profile_report().items()}


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[v.itemsize])


def _check_gathered(out_table, cols, idx):
    """Every column of the result is the input's column gathered at idx, bit for bit (a row is copied whole)."""
    got = out_table.columns()
    assert len(got) == len(cols)
    for g, c in zip(got, cols):
        gv, gm = g.to_numpy()
        gv = np.asarray(gv)
        gm = np.ones(len(gv), dtype=bool) if gm is None else np.asarray(gm, dtype=bool)
        hv, hm = R._rows(c)
        assert np.array_equal(gm, hm[idx])
        assert np.array_equal(np.where(gm, _bits(gv), 0), np.where(hm[idx], _bits(hv.astype(gv.dtype))[idx], 0))


# ---------------------------------------------------------------- golden vectors
@pytest.mark.parametrize("kind,c,ty", ORDER_CASES, ids=lambda x: x["name"] if isinstance(x, dict) else x)
def test_golden_orders(G, kind, c, ty):
    """sorted_order, sort and sort_by_key and their stable forms give the reference's stable expectation."""
    from cudf_amd import sorting as S
    cols = R.golden_table(c["input"], ty)
    n = cols[0].size
    o, no = _enums(c["orders"], c["null_orders"])
    expect = np.array(R.golden_expect(c, ty), dtype=np.int64)
    t = _table(G, cols)
    for order_fn, sort_fn, by_key_fn in ((S.sorted_order, S.sort, S.sort_by_key),
                                         (S.stable_sorted_order, S.stable_sort, S.stable_sort_by_key)):
        got = _indices(order_fn(t, o, no), n)
        assert got.tolist() == R.sorted_order(cols, c["orders"], c["null_orders"]).tolist()
        if c.get("compare") != "gathered":  # (otherwise the reference pins the gathered rows, checked below)
            assert got.tolist() == expect.tolist()
        for out in (sort_fn(t, o, no), by_key_fn(t, t, o, no)):
            assert out.num_rows() == n
            _check_gathered(out, cols, expect)
            assert S.is_sorted(out, o, no)


@pytest.mark.parametrize("c", GOLD["is_sorted"], ids=lambda c: c["name"])
def test_golden_is_sorted(G, c):
    from cudf_amd import sorting as S
    o, no = _enums(c["orders"], c["null_orders"])
    for ty in R.NUMERIC_CHRONO:
        assert S.is_sorted(_table(G, R.is_sorted_columns(GOLD, c, ty)), o, no) == c["expect"], ty


# ---------------------------------------------------------------- random tables against the restatement
FLOAT_POOL = [0.0, -0.0, np.inf, -np.inf, np.nan, -1.5, 2.25, 1e30, -3e-5]


def _rand_col(rng, ty, n, nullable, offset=0, universe=6):
    from oracle.oracle import NP_OF_TYPE_ID, TYPE_ID, HostColumn
    npt = np.dtype(NP_OF_TYPE_ID[TYPE_ID[ty]])
    m = n + offset
    if npt.kind == "b":
        data = rng.random(m) < 0.5
    elif npt.kind == "f":
        data = np.array(FLOAT_POOL, dtype=npt)[rng.integers(0, len(FLOAT_POOL), m)]
        bits = data.view(np.uint32 if npt.itemsize == 4 else np.uint64)
        odd = np.isnan(data) & (rng.random(m) < 0.5)  # other NaN bit patterns: the sign set, a payload bit set
        bits[odd] |= (bits.dtype.type(1) << bits.dtype.type(8 * npt.itemsize - 1)) | bits.dtype.type(5)
    else:
        lo = -(universe // 2) if npt.kind == "i" else 0
        data = rng.integers(lo, lo + universe, m).astype(npt)
    valid = rng.random(m) < 0.8 if nullable else None
    return HostColumn(data, valid, ty, offset=offset)


@functools.lru_cache(maxsize=None)
def _random_case(n, seed):
    """(columns, orders, null_orders, the restatement's order): made once, shared by the tests that use it."""
    rng = np.random.default_rng(1000 * seed + n)
    ncols = int(rng.integers(1, 5))
    cols = [_rand_col(rng, TYPES[rng.integers(len(TYPES))], n, rng.random() < 1 / 3) for _ in range(ncols)]
    orders = ["desc" if rng.random() < 0.5 else "asc" for _ in cols]
    null_orders = ["after" if rng.random() < 0.5 else "before" for _ in cols]
    expect = R.sorted_order(cols, orders, null_orders)
    expect.setflags(write=False)
    return cols, orders, null_orders, expect


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("n", ROWS)
def test_random_tables(G, n, seed):
    """The order equals the restatement's exactly (both are stable); sort gathers whole rows; its output is sorted."""
    from cudf_amd import sorting as S
    cols, orders, null_orders, expect = _random_case(n, seed)
    o, no = _enums(orders, null_orders)
    t = _table(G, cols)
    assert _indices(S.sorted_order(t, o, no), n).tolist() == expect.tolist()
    assert _indices(S.stable_sorted_order(t, o, no), n).tolist() == expect.tolist()
    out = S.sort(t, o, no)
    assert out.num_rows() == n and out.num_columns() == len(cols)
    if n:
        _check_gathered(out, cols, expect.astype(np.int64))
    assert S.is_sorted(out, o, no)
    assert S.is_sorted(t, o, no) == R.is_sorted(cols, orders, null_orders)


# ---------------------------------------------------------------- plan shapes, by the kernels that ran
def _shape_cases():
    from oracle.oracle import HostColumn
    rng = np.random.default_rng(5)
    n = 8192
    some = rng.random(n) < 0.9
    i32 = lambda: rng.integers(-2**31, 2**31, n).astype(np.int32)  # both signs, every byte varying
    i8 = lambda: rng.integers(-128, 128, n).astype(np.int8)
    return {
        # name: (columns, orders, fills, passes: exact / ("max", k) / None for whatever the restatement predicts)
        "int32_int32": ([HostColumn(i32()), HostColumn(i32())], [], 1, 8),
        "int32_nullable_int32_65_bits": ([HostColumn(i32()), HostColumn(i32(), some)], [], 2, None),
        "nullable_int64": ([HostColumn(rng.integers(-2**63, 2**63, n).astype(np.int64), some)], [], 2, None),
        "bool_int8_nullable_int16_desc_26_bits": ([HostColumn(rng.random(n) < 0.5), HostColumn(i8()),
                                                   HostColumn(rng.integers(-2**15, 2**15, n).astype(np.int16), some)],
                                                  ["asc", "asc", "desc"], 1, ("max", 4)),
        "16_int8": ([HostColumn(i8()) for _ in range(16)], [], 2, None),
        "all_rows_equal": ([HostColumn(np.full(n, -7, dtype=np.int32)), HostColumn(np.full(n, 2.5))], [], 2, 0),  # 96 bits
        "int32_in_0_200": ([HostColumn(rng.integers(0, 200, n).astype(np.int32))], [], 1, 1),
    }


@pytest.mark.parametrize("name", list(_shape_cases()))
def test_plan_shapes(G, name):
    """The fills (sort_pack_words) and radix passes (sort_scatter) each key shape costs equal what the documented layout predicts."""
    from cudf_amd import sorting as S
    cols, orders, fills, passes = _shape_cases()[name]
    words = R.packed_words(cols, orders)
    predicted = R.expected_passes(words)
    assert len(words) == fills
    if isinstance(passes, tuple):
        assert predicted <= passes[1]
    elif passes is not None:
        assert predicted == passes
    if name == "nullable_int64":
        assert R.expected_passes(words[1:]) == 1  # the second word is the null bit
    o, no = _enums(orders, [])
    t = _table(G, cols)
    idx, k = _kernels_of(lambda: _indices(S.sorted_order(t, o, no), cols[0].size))
    print(name, "fills", k.get("sort_pack_words", 0), "passes", k.get("sort_scatter", 0), "predicted", len(words), predicted)
    assert k.get("sort_pack_words", 0) == fills and k.get("sort_scatter", 0) == predicted, k
    assert k.get("sort_hist", 0) == predicted and not k.get("sort_words"), k
    assert idx.tolist() == R.sorted_order(cols, orders).tolist()  # (all rows equal: the identity order)


# ---------------------------------------------------------------- other cases
def test_sliced_columns_and_payload(G):
    """Key columns with non-zero offsets whose mask offsets are no multiple of 32, payload columns through sort_by_key."""
    from cudf_amd import sorting as S
    rng = np.random.default_rng(21)
    n = 5000
    keys = [_rand_col(rng, "int16", n, True, offset=7), _rand_col(rng, "float64", n, True, offset=45),
            _rand_col(rng, "uint32", n, False, offset=3)]
    payload = [_rand_col(rng, "float64", n, True, offset=13, universe=10**6), _rand_col(rng, "int8", n, False, offset=1, universe=200)]
    orders, null_orders = ["desc", "asc", "desc"], ["after", "after", "before"]
    o, no = _enums(orders, null_orders)
    expect = R.sorted_order(keys, orders, null_orders)
    assert _indices(S.sorted_order(_table(G, keys), o, no), n).tolist() == expect.tolist()
    for fn in (S.sort_by_key, S.stable_sort_by_key):
        out = fn(_table(G, payload), _table(G, keys), o, no)
        _check_gathered(out, payload, expect.astype(np.int64))


def test_non_default_stream(G):
    import torch

    from cudf_amd import sorting as S
    cols, orders, null_orders, expect = _random_case(12289, 1)
    o, no = _enums(orders, null_orders)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = _table(G, cols)
        idx = S.sorted_order(t, o, no, stream=s)
        out = S.sort(t, o, no, stream=s)
        ok = S.is_sorted(out, o, no, stream=s)
    s.synchronize()
    assert _indices(idx, 12289).tolist() == expect.tolist() and ok


def test_rejected_inputs(G):
    from cudf_amd import sorting as S
    from cudf_amd.types import NullOrder, Order
    from oracle.oracle import HostColumn
    t = _table(G, [HostColumn(np.arange(10, dtype=np.int32)), HostColumn(np.arange(10, dtype=np.int64))])
    short = _table(G, [HostColumn(np.arange(9, dtype=np.int32))])
    wide = _table(G, [HostColumn(np.arange(10, dtype=np.int32)) for _ in range(17)])  # beyond the device tables' 16 columns
    for call in (lambda: S.sorted_order(t, [Order.ASCENDING]),
                 lambda: S.sort(t, [Order.ASCENDING] * 3),
                 lambda: S.sort_by_key(t, t, [Order.DESCENDING]),
                 lambda: S.is_sorted(t, [Order.ASCENDING], []),
                 lambda: S.stable_sorted_order(t, [], [NullOrder.AFTER]),
                 lambda: S.stable_sort(t, [Order.ASCENDING] * 2, [NullOrder.AFTER] * 3),
                 lambda: S.is_sorted(t, [], [NullOrder.BEFORE]),
                 lambda: S.sort_by_key(t, short),
                 lambda: S.stable_sort_by_key(short, t),
                 lambda: S.sorted_order(wide),
                 lambda: S.is_sorted(wide)):
        with pytest.raises(_lib_error()) as e:
            call()
        assert not isinstance(e.value, (ValueError, TypeError, IndexError, MemoryError))  # the logic-error status


def _lib_error():
    from cudf_amd import _lib
    return _lib.CudfAmdError


def test_no_key_columns_and_no_rows(G):
    from cudf_amd import sorting as S
    from oracle.oracle import HostColumn
    import cudf_amd
    empty = _table(G, [HostColumn(np.zeros(0, dtype=np.int64)), HostColumn(np.zeros(0, dtype=np.float32))])
    assert S.sorted_order(empty).size() == 0
    out = S.sort(empty)
    assert out.num_columns() == 2 and out.num_rows() == 0
    assert [c.type().id().name for c in out.columns()] == ["INT64", "FLOAT32"]
    assert S.is_sorted(empty) and S.is_sorted(cudf_amd.Table([]))
    assert S.sorted_order(cudf_amd.Table([])).size() == 0


# ---------------------------------------------------------------- is_sorted at its edges
@pytest.mark.parametrize("at", [0, 63, 64, 4095, 4096, 12287], ids=lambda a: f"rows_{a}_{a + 1}")
def test_is_sorted_one_swapped_pair(G, at):
    """True on a sorted table with ties; false after one adjacent pair of distinct rows is swapped at row 0/1, at a wave edge, at a
    tile edge and at the last two rows."""
    from cudf_amd import sorting as S
    from oracle.oracle import HostColumn
    n = 12289
    a = (np.arange(n) // 2).astype(np.int32)  # pairs of equal adjacent values
    b = -np.arange(n, dtype=np.float64)       # descending inside and across the pairs
    o, no = _enums(["asc", "desc"], [])
    assert S.is_sorted(_table(G, [HostColumn(a), HostColumn(a.astype(np.int64))]), [], [])  # equal adjacent rows are sorted
    assert S.is_sorted(_table(G, [HostColumn(a), HostColumn(b)]), o, no)
    b2 = b.copy()
    b2[[at, at + 1]] = b2[[at + 1, at]]
    a2 = a.copy()
    a2[[at, at + 1]] = a2[[at + 1, at]]
    assert not S.is_sorted(_table(G, [HostColumn(a2), HostColumn(b2)]), o, no)
    assert R.is_sorted([HostColumn(a2), HostColumn(b2)], ["asc", "desc"], []) is False


# ---------------------------------------------------------------- 16M rows
@pytest.mark.parametrize("shape", ["int64", "int32_float32_desc_nulls_after"])
def test_16m_rows(G, shape):
    import torch

    import cudf_amd
    from cudf_amd import sorting as S
    from cudf_amd.types import NullOrder, Order
    n = 16 * 1024 * 1024
    gen = torch.Generator(device="cuda").manual_seed(3)
    if shape == "int64":
        k = torch.randint(-2**40, 2**40, (n,), device="cuda", dtype=torch.int64, generator=gen)
        t = cudf_amd.Table([cudf_amd.Column.from_torch(k)])
        o, no = [], []
    else:
        a = torch.randint(-1000, 1000, (n,), device="cuda", dtype=torch.int32, generator=gen)
        b = torch.randn((n,), device="cuda", dtype=torch.float32, generator=gen)
        t = cudf_amd.Table([cudf_amd.Column.from_torch(a), cudf_amd.Column.from_torch(b)])
        o, no = [Order.ASCENDING, Order.DESCENDING], [NullOrder.AFTER, NullOrder.AFTER]
    idx = S.sorted_order(t, o, no).to_torch()
    assert idx.numel() == n and int(idx.min()) >= 0 and int(idx.max()) < n
    assert bool((torch.bincount(idx.to(torch.int64), minlength=n) == 1).all())  # a permutation
    assert S.is_sorted(S.sort(t, o, no), o, no)
    if shape == "int64":
        assert torch.equal(idx.to(torch.int64), torch.sort(k, stable=True).indices)
    torch.cuda.synchronize()
