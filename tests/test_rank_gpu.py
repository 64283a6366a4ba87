"""GPU tests of cudf::rank through the C ABI and cudf_amd.sorting.rank: the golden vectors (tests/golden/kat_rank.json) over the
sorting tests' types, seeded random columns against the numpy restatement (tests/rank_restatement.py) at the wave, radix-tile
and rank-tile edges, run shapes that cross the rank kernels' tile edges, the plan shapes proven by the kernels that ran, sliced
and all-valid masks, a second stream, the rejected enum values and one 4M-row column. Every comparison is exact: the restatement's
only floating-point steps are min + (count - 1) / 2.0 and one division, correctly rounded on both sides."""
import ctypes as C
import functools

import numpy as np
import pytest

import rank_restatement as R
import sorting_restatement as S

pytestmark = pytest.mark.gpu

GOLD = R.load_golden()
T = 2048  # the rank kernels' tile (RANK_TILE of cudf_amd/csrc/sorting/sorting_impl.hpp; tests/test_rank_abi.py pins it)
TYPES = ["int8", "int16", "int32", "int64", "uint32", "uint64", "float32", "float64", "bool", "decimal64"]  # the sorting tests' list
ROWS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 12289, T - 1, T, T + 1, 3 * T + 1]
RANDOM_TYPES = ["int8", "int32", "int64", "uint64", "float32", "float64", "bool", "decimal64"]
FLOAT_POOL = [0.0, -0.0, np.inf, -np.inf, np.nan, -1.5, 2.25, 1e30, -3e-5]  # as the sorting tests'
ALL_CALLS = [(m, o, p, no, pct) for m in R.METHODS for (o, p, no) in R.DEFINED for pct in (False, True)]


@pytest.fixture(scope="module")
def G(gpu):
    import gpu_backend
    return gpu_backend


def _rank(col, method, order, policy, null_order, pct, stream=None):
    from cudf_amd import sorting
    from cudf_amd.aggregation import RankMethod
    from cudf_amd.types import NullOrder, NullPolicy, Order
    return sorting.rank(col, RankMethod[method.upper()], Order.DESCENDING if order == "desc" else Order.ASCENDING,
                        NullPolicy.INCLUDE if policy == "include" else NullPolicy.EXCLUDE,
                        NullOrder.BEFORE if null_order == "before" else NullOrder.AFTER, pct, stream=stream)


def _check(got, expect, n, what=None):
    """The type id, the size, the mask, the null count and every value that is valid, bit for bit."""
    values, valid = expect
    assert got.type().id().name == ("FLOAT64" if values.dtype == np.float64 else "INT32"), what
    assert got.size() == n, what
    data, mask = got.to_numpy()
    data = np.asarray(data)
    if valid is None:
        assert mask is None and got.null_count() == 0, what
        assert np.array_equal(data, values), what
    else:
        assert mask is not None and np.array_equal(np.asarray(mask, dtype=bool), valid), what
        assert got.null_count() == int((~valid).sum()), what
        assert np.array_equal(data[valid], values[valid]), what


def _check_all_calls(G, host, calls=ALL_CALLS):
    dev = G.to_device(host)
    for call in calls:
        _check(_rank(dev, *call), R.rank(host, *call), host.size, call)


def _kernels_of(fn):
    from cudf_amd import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
    finally:
        _lib.profile_enable(False)
    return out, {k: v[0] for k, v in _lib.profile_report().items()}


# ---------------------------------------------------------------- golden vectors
GOLDEN_TYPES = [t for t in TYPES if t != "bool"]  # (the reference's suite skips bool: rank_test.cpp:74)


@pytest.mark.parametrize("case", list(R.golden_cases(GOLD)), ids=lambda c: f"{c[0]}-{c[1]}")
def test_golden_cases(G, case):
    _, col, method, order, policy, null_order, pct, values, valid = case
    dtype = np.float64 if pct or method == "average" else np.int32
    expect = (np.array(values, dtype=dtype), None if valid is None else np.array(valid, dtype=bool))
    for ty in GOLDEN_TYPES:
        host = R.golden_column(GOLD, col, ty)
        _check(_rank(G.to_device(host), method, order, policy, null_order, pct), expect, host.size, ty)


def test_golden_large(G):
    from oracle.oracle import HostColumn
    g = GOLD["large"]
    host = HostColumn(np.arange(g["rows"], dtype=np.int64))
    got = _rank(G.to_device(host), g["method"], g["order"], g["policy"], g["null_order"], False)
    _check(got, (np.arange(1, g["rows"] + 1, dtype=np.float64), None), g["rows"])


@pytest.mark.parametrize("d", GOLD["documented"], ids=lambda d: d["name"])
def test_documented_examples(G, d):
    host = S.host_column("int32", d["values"], d.get("valid"))
    dev = G.to_device(host)
    for method, expect in d["expect"].items():
        valid = np.array(d["valid"], dtype=bool) if "valid" in d and d["policy"] == "exclude" else None
        values = np.array(expect, dtype=np.float64 if method == "average" else np.int32)
        _check(_rank(dev, method, "asc", d["policy"], d["null_order"], False), (values, valid), host.size, method)


# ---------------------------------------------------------------- random columns against the restatement
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


@pytest.mark.parametrize("ty", RANDOM_TYPES)
@pytest.mark.parametrize("n", ROWS)
def test_random_columns(G, n, ty):
    """Every method, defined (order, policy, precedence) and percentage, without and with nulls; few distinct values, so the runs
    are long, and a second universe of n / 3 values, so most runs are short."""
    rng = np.random.default_rng(7 * n + len(ty))
    for nullable in (False, True):
        _check_all_calls(G, _rand_col(rng, ty, n, nullable))
    few = [c for c in ALL_CALLS if c[0] in ("average", "dense") and c[4]]
    _check_all_calls(G, _rand_col(rng, ty, n, True, universe=max(2, n // 3)), few)


# ---------------------------------------------------------------- run shapes that cross the tile edges
def _runs(lengths, ty="int32", nulls=0, seed=0):
    """A shuffled column whose sorted order has runs of these lengths (ascending values), then `nulls` null rows."""
    from oracle.oracle import HostColumn
    values = np.repeat(np.arange(len(lengths), dtype=np.int64) * 3 - 5, np.array(lengths, dtype=np.int64))
    data = np.concatenate([values, np.zeros(nulls, dtype=np.int64)])
    valid = np.concatenate([np.ones(len(values), dtype=bool), np.zeros(nulls, dtype=bool)])
    perm = np.random.default_rng(seed).permutation(len(data))
    return HostColumn(data[perm].astype(ty), valid[perm] if nulls else None, ty)


RUN_SHAPES = {
    "all_rows_equal": lambda: [_runs([3 * T + 5]), _runs([3 * T + 5], "int64")],
    "all_rows_null": lambda: [_runs([], "int32", 2 * T + 3), _runs([], "int64", 2 * T + 3)],
    "every_row_distinct": lambda: [_runs([1] * (3 * T + 1))],
    "runs_of_a_tile_aligned": lambda: [_runs([T, T, T]), _runs([T, T, T], "float64", 1)],
    "runs_of_a_tile_shifted_by_one": lambda: [_runs([1, T, T, T - 1]), _runs([1, T, T, 5], "int64", 3)],
    "lone_values_at_a_tile_edge": lambda: [_runs([T - 1, 1, 1, T - 1, 1, 1, 7]), _runs([T - 1, 1, 1, T - 1], "int64", 2)],
    "null_block_at_a_tile_edge": lambda: [_runs([5] * k + [T - 5 * k + d], ty, T + 9)
                                           for ty, k in (("int32", 3), ("int64", 40)) for d in (-1, 0, 1)],
    "null_block_of_a_tile": lambda: [_runs([3, 4, 50], ty, T + d) for ty in ("int32", "float64") for d in (-1, 0, 1)],
    "run_over_three_tiles": lambda: [_runs([T - 5, T + 10, 7]), _runs([100, 3 * T, 100], "int64", 1), _runs([T - 1, 2 * T + 2])],
}


@pytest.mark.parametrize("shape", list(RUN_SHAPES))
def test_run_shapes(G, shape):
    """The nulls sort last or first with the call, so a null block of T - 1, T or T + 1 rows both starts and ends at a tile edge."""
    for host in RUN_SHAPES[shape]():
        _check_all_calls(G, host)


# ---------------------------------------------------------------- plan shapes, by the kernels that ran
def _plan_cases():
    from oracle.oracle import HostColumn
    rng = np.random.default_rng(11)
    n = 8192
    some = rng.random(n) < 0.9
    return {
        # name: (column, words of the plan)
        "nullable_int64": (HostColumn(rng.integers(-50, 50, n).astype(np.int64), some), 2),
        "nullable_float64": (HostColumn(rng.integers(-50, 50, n) / 4.0, some), 2),
        "nullable_int32": (HostColumn(rng.integers(-50, 50, n).astype(np.int32), some), 1),
        "int64": (HostColumn(rng.integers(-50, 50, n).astype(np.int64)), 1),
    }


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("name", list(_plan_cases()))
def test_plan_shapes_and_launches(G, name, method):
    """Beyond the sort's own kernels FIRST is one launch and reads no words, MIN / MAX / AVERAGE one launch (and one refill of
    the value word for the two-word plan), DENSE the count and apply kernels and one scan."""
    host, nwords = _plan_cases()[name]
    assert len(S.packed_words([host], ["asc"], ["after"])) == nwords
    dev = G.to_device(host)
    for pct in (False, True):
        got, k = _kernels_of(lambda: _rank(dev, method, "asc", "include", "after", pct))
        _check(got, R.rank(host, method, "asc", "include", "after", pct), host.size)
        ran = {kernel: k.get(kernel, 0) for kernel in ("rank_first", "rank_ties", "rank_dense_count", "rank_dense_apply")}
        refill = 1 if nwords == 2 and method != "first" else 0
        assert k.get("sort_pack_words", 0) == nwords + refill, k
        assert k.get("sort_scatter", 0) == k.get("sort_hist", 0) > 0, k
        if method == "first":
            assert ran == {"rank_first": 1, "rank_ties": 0, "rank_dense_count": 0, "rank_dense_apply": 0}, k
        elif method == "dense":
            assert ran == {"rank_first": 0, "rank_ties": 0, "rank_dense_count": 1, "rank_dense_apply": 1}, k
        else:
            assert ran == {"rank_first": 0, "rank_ties": 1, "rank_dense_count": 0, "rank_dense_apply": 0}, k
        assert k.get("sort_scan", 0) == k["sort_scatter"] + (1 if method == "dense" else 0), k  # one scan per radix pass


# ---------------------------------------------------------------- other inputs
def test_sliced_input_with_a_mask(G):
    """offset > 0 and no multiple of 32: the result's mask starts at bit 0 and carries the slice's null count."""
    rng = np.random.default_rng(3)
    for ty in ("int32", "float64"):
        host = _rand_col(rng, ty, 5000, True, offset=37)
        _check_all_calls(G, host, [c for c in ALL_CALLS if c[2] == "exclude"])
        _check_all_calls(G, host, [("min", "asc", "include", "before", False), ("dense", "desc", "include", "after", True)])


def test_mask_without_nulls(G):
    """EXCLUDE keeps a mask that has no nulls (null count 0); INCLUDE returns none; a column without a mask never gets one."""
    from oracle.oracle import HostColumn
    rng = np.random.default_rng(4)
    n = T + 100
    for data in (rng.integers(-4, 4, n).astype(np.int64), rng.integers(-4, 4, n).astype(np.int16)):
        host = HostColumn(data, np.ones(n, dtype=bool))
        _check_all_calls(G, host)
        got = _rank(G.to_device(host), "max", "asc", "exclude", "after", False)
        assert got.nullable() and got.null_count() == 0
        assert not _rank(G.to_device(host), "max", "asc", "include", "after", False).nullable()
        assert not _rank(G.to_device(HostColumn(data)), "max", "asc", "exclude", "after", False).nullable()


def test_non_default_stream(G):
    import torch
    rng = np.random.default_rng(5)
    host = _rand_col(rng, "float64", 12289, True)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = G.to_device(host)
        got = [(c, _rank(dev, *c, stream=s)) for c in ALL_CALLS if c[1] == "asc"]
    s.synchronize()
    for c, out in got:
        _check(out, R.rank(host, *c), host.size, c)


def test_enum_values_outside_their_range(G):
    from cudf_amd import _lib
    from oracle.oracle import HostColumn
    lib = _lib.load()
    view = G.to_device(HostColumn(np.arange(10, dtype=np.int32)))._view()
    ok = [0, 0, 0, 0, 0]  # method, column_order, null_handling, null_precedence, percentage
    out = C.c_void_p()
    assert lib.cudf_amd_rank(C.byref(view), *ok, None, C.byref(out)) == 0 and out.value
    lib.cudf_amd_table_free(out)
    for arg, bad in ((0, 5), (0, -1), (1, 2), (1, -1), (2, 2), (2, -1), (3, 2), (3, -1)):
        args = list(ok)
        args[arg] = bad
        out = C.c_void_p()
        assert lib.cudf_amd_rank(C.byref(view), *args, None, C.byref(out)) == 1, (arg, bad)  # CUDF_AMD_LOGIC_ERROR
        assert not out.value


def test_rejected_column_type(G):
    """A column that is not fixed-width fails as sorted_order's make_plan fails, empty or not."""
    import cudf_amd
    from cudf_amd import _lib
    from cudf_amd.types import DataType, TypeId
    from oracle.oracle import HostColumn
    dev = G.to_device(HostColumn(np.arange(4, dtype=np.int32)))
    strings = cudf_amd.Column(DataType(TypeId.STRING), 4, dev.data_ptr(), None, 0, 0, dev)
    with pytest.raises(_lib.CudfAmdError):
        _rank(strings, "min", "asc", "include", "after", False)
    with pytest.raises(_lib.CudfAmdError):
        cudf_amd.sorting.sorted_order(cudf_amd.Table([strings]))


# ---------------------------------------------------------------- 4M rows
@functools.lru_cache(maxsize=None)
def _large_case():
    from oracle.oracle import HostColumn
    rng = np.random.default_rng(9)
    n = 1 << 22
    pool = np.concatenate([rng.standard_normal(995), [0.0, -0.0, np.nan, np.inf, -np.inf]])
    return HostColumn(pool[rng.integers(0, len(pool), n)], rng.random(n) < 0.9)


@pytest.mark.parametrize("method", ["average", "dense"])
def test_4m_rows(G, method):
    """About 1,000 distinct values and 10 % nulls: every run spans tiles, and the null run spans about 200 of them."""
    host = _large_case()
    dev = G.to_device(host)
    for order, policy, null_order in (("asc", "exclude", "after"), ("desc", "include", "after")):
        _check(_rank(dev, method, order, policy, null_order, True), R.rank(host, method, order, policy, null_order, True), host.size)
