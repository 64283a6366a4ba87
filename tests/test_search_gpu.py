"""GPU tests of cudf::lower_bound / upper_bound through the C ABI and cudf_amd.search: the golden vectors
(tests/golden/kat_search.json), seeded random tables against the numpy restatement (tests/search_merge_restatement.py) at the
power-of-two edges of the binary search and the wave and workgroup edges of the needles, the shapes of the joint plan of the two
tables (a null bit forced on the side without a mask, the null bit in the next word, three words), floats, descending orders,
sliced columns, a second stream, 16 key columns, the rejected inputs and a 4M x 1M property against torch.searchsorted."""
import functools

import numpy as np
import pytest

import search_merge_restatement as R
import sorting_restatement as S
from test_sorting_gpu import _enums, _indices, _kernels_of, _lib_error, _rand_col, _table

pytestmark = pytest.mark.gpu

GOLD = R.load_golden("kat_search.json")
HAY_ROWS = [0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025]  # the binary search's power-of-two edges and the wave
NEEDLE_ROWS = [0, 1, 63, 64, 65, 257]                   # wave and workgroup edges
TYPES = ["int8", "int16", "int32", "int64", "uint32", "uint64", "float32", "float64", "bool", "decimal64"]


@pytest.fixture(scope="module")
def G(gpu):
    import gpu_backend
    return gpu_backend


def _both(G, hay, needles, orders, null_orders, stream=None):
    """(lower_bound, upper_bound) of the library as numpy arrays."""
    from cudf_amd import search
    o, no = _enums(orders, null_orders)
    h, n = _table(G, hay), _table(G, needles)
    rows = needles[0].size
    return (_indices(search.lower_bound(h, n, o, no, stream=stream), rows), _indices(search.upper_bound(h, n, o, no, stream=stream), rows))


def _check(G, hay, needles, orders, null_orders):
    lo, up = _both(G, hay, needles, orders, null_orders)
    assert lo.tolist() == R.lower_bound(hay, needles, orders, null_orders).tolist()
    assert up.tolist() == R.upper_bound(hay, needles, orders, null_orders).tolist()
    return lo, up


def _sorted(cols, orders, null_orders):
    return R.sort_table(cols, list(range(len(cols))), orders, null_orders)


# ---------------------------------------------------------------- golden vectors
@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: c["name"])
def test_golden(G, c):
    from cudf_amd import search
    fn = search.lower_bound if c["fn"] == "lower" else search.upper_bound
    o, no = _enums(c["orders"], c["null_orders"])
    for ty in (["int64"] if c["for"] == ["as_written"] else c["for"]):
        hay, needles = S.golden_table(c["haystack"], ty), S.golden_table(c["needles"], ty)
        got = _indices(fn(_table(G, hay), _table(G, needles), o, no), needles[0].size)
        assert got.tolist() == c["expect"], ty


# ---------------------------------------------------------------- random tables against the restatement
@functools.lru_cache(maxsize=None)
def _random_case(h, n, seed):
    rng = np.random.default_rng(100000 * seed + 1000 * h + n)
    ncols = int(rng.integers(1, 4))
    types = [TYPES[rng.integers(len(TYPES))] for _ in range(ncols)]
    orders = ["desc" if rng.random() < 0.5 else "asc" for _ in types]
    null_orders = ["after" if rng.random() < 0.5 else "before" for _ in types]
    hay = _sorted([_rand_col(rng, t, h, rng.random() < 0.4) for t in types], orders, null_orders)
    needles = [_rand_col(rng, t, n, rng.random() < 0.4) for t in types]
    return hay, needles, orders, null_orders


@pytest.mark.parametrize("n", NEEDLE_ROWS)
@pytest.mark.parametrize("h", HAY_ROWS)
def test_random_tables(G, h, n):
    for seed in range(2):
        lo, up = _check(G, *_random_case(h, n, seed))
        assert ((0 <= lo) & (lo <= up) & (up <= h)).all()


# ---------------------------------------------------------------- named cases
def _col(data, valid=None, ty=None, offset=0):
    from oracle.oracle import HostColumn
    return HostColumn(np.asarray(data), None if valid is None else np.asarray(valid, dtype=bool), ty, offset=offset)


def test_needles_outside_the_haystack(G):
    hay = [_col(np.arange(100, 1100, dtype=np.int32))]
    lo, up = _check(G, hay, [_col(np.arange(0, 70, dtype=np.int32))], [], [])
    assert not lo.any() and not up.any()  # every needle below the first row
    lo, up = _check(G, hay, [_col(np.arange(2000, 2070, dtype=np.int32))], [], [])
    assert (lo == 1000).all() and (up == 1000).all()  # every needle above the last row


def test_one_repeated_value(G):
    n = 1025
    lo, up = _check(G, [_col(np.full(n, 7, dtype=np.int64))], [_col(np.array([7, 6, 8, 7], dtype=np.int64))], [], [])
    assert lo.tolist() == [0, 0, n, 0] and up.tolist() == [n, 0, n, n]


@pytest.mark.parametrize("nullable_side", ["needles", "haystack"])
def test_null_bit_forced_on_the_side_without_a_mask(G, nullable_side):
    """(int32, int32) keys: either table alone packs into one 64-bit word, the joint layout (one null bit) needs two. Plans made for
    each table separately would compare words of different layouts."""
    rng = np.random.default_rng(7)
    h, n = 1025, 257
    mask = lambda m: rng.random(m) < 0.7
    hv = mask(h) if nullable_side == "haystack" else None
    nv = mask(n) if nullable_side == "needles" else None
    for null_orders in (["before", "before"], ["after", "after"]):
        hay = _sorted([_col(rng.integers(-3, 3, h).astype(np.int32)), _col(rng.integers(-3, 3, h).astype(np.int32), hv)], [], null_orders)
        needles = [_col(rng.integers(-3, 3, n).astype(np.int32)), _col(rng.integers(-3, 3, n).astype(np.int32), nv)]
        assert len(S.packed_words(hay if hv is None else needles)) == 1  # the side without nulls alone: one word
        (lo, up), k = _kernels_of(lambda: _check(G, hay, needles, [], null_orders))
        assert k.get("bound_search") == 2 and not k.get("sort_pack_words"), k


def test_nullable_int64_null_bit_in_the_next_word(G):
    rng = np.random.default_rng(8)
    big = lambda m: rng.integers(-2**62, 2**62, m).astype(np.int64) | 1
    for null_orders in (["before"], ["after"]):
        hay = _sorted([_col(big(1000), rng.random(1000) < 0.8)], [], null_orders)
        hv, _ = S._rows(hay[0])
        needles = [_col(np.concatenate([np.asarray(hv)[::7], big(50)]), rng.random(143 + 50) < 0.8)]
        _check(G, hay, needles, [], null_orders)
        plain = np.sort(big(1000))
        _check(G, [_col(plain)], [_col(np.concatenate([plain[::9], plain[:5] - 1]))], [], [])  # 64 bits, no null bit: one word


@pytest.mark.parametrize("first,words", [("int32", 3), ("int64", 4)])
def test_several_words_the_last_decides(G, first, words):
    """(first, nullable int64, int32): the int32 is word 0, the int64's value word 1, its null bit word 2 - shared with an int32
    first column, while an int64 first column takes a fourth word. The most significant words tie; the least significant decides."""
    rng = np.random.default_rng(9)
    h = 1000
    a = np.full(h, 5, dtype=first)
    b, bv = np.full(h, -2, dtype=np.int64), np.ones(h, dtype=bool)
    bv[:10] = False
    c = np.sort(rng.integers(-1000, 1000, h - 10).astype(np.int32))
    hay = [_col(a), _col(b, bv), _col(np.concatenate([np.sort(rng.integers(-9, 9, 10).astype(np.int32)), c]))]
    n = 130
    needles = [_col(np.full(n, 5, dtype=first)), _col(np.full(n, -2, dtype=np.int64), rng.random(n) < 0.9),
               _col(rng.integers(-1000, 1000, n).astype(np.int32))]
    assert len(S.packed_words(hay)) == words and S.is_sorted(hay)
    lo, up = _check(G, hay, needles, [], [])
    assert len(set(lo.tolist())) > 50


def test_float_keys(G):
    """_rand_col draws floats from test_sorting_gpu.FLOAT_POOL: both zeros, both infinities, NaNs of several bit patterns."""
    rng = np.random.default_rng(10)
    for ty in ("float32", "float64"):
        for orders, null_orders in ((["asc"], ["before"]), (["desc"], ["after"])):
            hay = _sorted([_rand_col(rng, ty, 300, True)], orders, null_orders)
            needles = [_rand_col(rng, ty, 100, True)]
            _check(G, hay, needles, orders, null_orders)


@pytest.mark.parametrize("null_order", ["before", "after"])
def test_descending(G, null_order):
    rng = np.random.default_rng(11)
    orders, null_orders = ["desc", "desc"], [null_order] * 2
    hay = _sorted([_rand_col(rng, "int16", 500, True), _rand_col(rng, "uint64", 500, True)], orders, null_orders)
    needles = [_rand_col(rng, "int16", 130, True), _rand_col(rng, "uint64", 130, True)]
    _check(G, hay, needles, orders, null_orders)


def test_sliced_columns(G):
    """Offsets that are no multiple of 32 and differ between the two tables."""
    rng = np.random.default_rng(12)
    orders, null_orders = ["asc", "desc"], ["after", "before"]
    body = _sorted([_rand_col(rng, "int32", 700, True), _rand_col(rng, "float64", 700, True)], orders, null_orders)

    def shifted(c, off):
        v, m = S._rows(c)
        pad_v = np.concatenate([np.full(off, 99, dtype=np.asarray(v).dtype), np.asarray(v)])
        return _col(pad_v, np.concatenate([rng.random(off) < 0.5, m]), R._type_name(c), offset=off)
    hay = [shifted(body[0], 7), shifted(body[1], 45)]
    needles = [_rand_col(rng, "int32", 200, True, offset=13), _rand_col(rng, "float64", 200, False, offset=3)]
    _check(G, hay, needles, orders, null_orders)


def test_non_default_stream(G):
    import torch
    hay, needles, orders, null_orders = _random_case(1025, 257, 0)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        lo, up = _both(G, hay, needles, orders, null_orders, stream=s)
    s.synchronize()
    assert lo.tolist() == R.lower_bound(hay, needles, orders, null_orders).tolist()
    assert up.tolist() == R.upper_bound(hay, needles, orders, null_orders).tolist()


def test_16_key_columns(G):
    """16 nullable int64 columns: 32 words, the kernel that keeps no needle words."""
    rng = np.random.default_rng(13)
    orders = ["desc" if i % 3 == 0 else "asc" for i in range(16)]
    null_orders = ["after" if i % 2 else "before" for i in range(16)]
    hay = _sorted([_rand_col(rng, "int64", 600, True, universe=2) for _ in range(16)], orders, null_orders)
    needles = [_rand_col(rng, "int64", 150, True, universe=2) for _ in range(16)]
    assert len(S.packed_words(hay)) == 32
    _check(G, hay, needles, orders, null_orders)
    mixed = ["int8"] * 16  # 16 narrow columns: two words
    hay = _sorted([_rand_col(rng, t, 600, False, universe=3) for t in mixed], [], [])
    _check(G, hay, [_rand_col(rng, t, 150, False, universe=3) for t in mixed], [], [])


def test_kernels_by_profiler_scope(G):
    hay, needles = [_col(np.arange(100, dtype=np.int32))], [_col(np.arange(0, 100, 3, dtype=np.int32))]
    _, k = _kernels_of(lambda: _both(G, hay, needles, [], []))
    assert k.get("bound_search") == 2 and not k.get("sort_pack_words") and not k.get("sort_scatter"), k
    _, k = _kernels_of(lambda: _both(G, [_col(np.zeros(0, dtype=np.int32))], needles, [], []))
    assert not k.get("bound_search"), k  # no haystack rows: no search


# ---------------------------------------------------------------- rejected and trivial inputs
def test_rejected_inputs(G):
    from cudf_amd import search
    from cudf_amd.types import NullOrder, Order
    two = lambda n: _table(G, [_col(np.arange(n, dtype=np.int32)), _col(np.arange(n, dtype=np.int64))])
    t, empty = two(10), two(0)
    wide = _table(G, [_col(np.arange(4, dtype=np.int32)) for _ in range(17)])
    for fn in (search.lower_bound, search.upper_bound):
        for call in (lambda: fn(t, t, [Order.ASCENDING]),
                     lambda: fn(t, t, [Order.ASCENDING] * 3, []),
                     lambda: fn(t, t, [], [NullOrder.AFTER]),
                     lambda: fn(empty, t, [Order.ASCENDING]),          # before the shortcuts
                     lambda: fn(t, empty, [], [NullOrder.BEFORE] * 3),
                     lambda: fn(empty, empty, [Order.DESCENDING]),
                     lambda: fn(wide, wide)):
            with pytest.raises(_lib_error()) as e:
                call()
            assert not isinstance(e.value, (ValueError, TypeError, IndexError, MemoryError))  # the logic-error status
        one = _table(G, [_col(np.arange(10, dtype=np.int32))])
        other = _table(G, [_col(np.arange(10, dtype=np.int32)), _col(np.arange(10, dtype=np.float64))])
        for call in (lambda: fn(t, one), lambda: fn(one, t), lambda: fn(t, other), lambda: fn(empty, other)):
            with pytest.raises(ValueError):  # std::invalid_argument, as the joins map it
                call()


def test_no_rows(G):
    from cudf_amd import search
    t = _table(G, [_col(np.arange(10, dtype=np.int32))])
    empty = _table(G, [_col(np.zeros(0, dtype=np.int32))])
    for fn in (search.lower_bound, search.upper_bound):
        assert _indices(fn(empty, t), 10).tolist() == [0] * 10
        assert fn(t, empty).size() == 0 and fn(empty, empty).size() == 0


# ---------------------------------------------------------------- 4M x 1M
def test_4m_haystack_1m_needles(G):
    import torch

    import cudf_amd
    from cudf_amd import search
    gen = torch.Generator(device="cuda").manual_seed(5)
    hay = torch.sort(torch.randint(-2**40, 2**40, (4 * 1024 * 1024,), device="cuda", dtype=torch.int64, generator=gen)).values
    hay[1000:3000] = hay[1000]  # a run of equal rows
    needles = torch.randint(-2**40, 2**40, (1024 * 1024,), device="cuda", dtype=torch.int64, generator=gen)
    needles[:4096] = hay[torch.randint(0, hay.numel(), (4096,), device="cuda", generator=gen)]  # needles that are present
    needles[4096] = hay[1000]  # and one inside the run
    h, n = cudf_amd.Table([cudf_amd.Column.from_torch(hay)]), cudf_amd.Table([cudf_amd.Column.from_torch(needles)])
    lo = search.lower_bound(h, n).to_torch()
    up = search.upper_bound(h, n).to_torch()
    assert torch.equal(lo.to(torch.int64), torch.searchsorted(hay, needles, right=False))
    assert torch.equal(up.to(torch.int64), torch.searchsorted(hay, needles, right=True))
    assert int((up - lo).max()) >= 2000
    torch.cuda.synchronize()
