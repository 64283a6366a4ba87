"""GPU tests of cudf::merge through the C ABI and cudf_amd.merge. Every result goes through merge_check of
tests/search_merge_restatement.py (the output keys are sorted, its rows are the inputs' rows, each input's rows keep their order) and
through cudf_amd.sorting.is_sorted: the golden vectors (tests/golden/kat_merge.json), two-table merges of seeded random sorted
tables at the wave and workgroup edges with a key universe of 6, masks on one side only, key columns that are not the first, N-way
merges, the shortcuts, every rejected input, a 2 x 2M-row property against torch.sort and the kernels that ran."""
import functools
import itertools

import numpy as np
import pytest

import search_merge_restatement as R
import sorting_restatement as S
from test_sorting_gpu import _enums, _kernels_of, _lib_error, _rand_col, _table

pytestmark = pytest.mark.gpu

GOLD = R.load_golden("kat_merge.json")
SIZES = list(itertools.product([0, 1, 63, 64, 65, 1025], [0, 1, 64, 1025, 4097]))


@pytest.fixture(scope="module")
def G(gpu):
    import gpu_backend
    return gpu_backend


def _host(table):
    """The columns of a device Table as HostColumns."""
    from oracle.oracle import TYPE_ID, HostColumn
    names = {v: k for k, v in TYPE_ID.items()}
    out = []
    for c in table.columns():
        v, m = c.to_numpy()
        out.append(HostColumn(np.asarray(v), None if m is None else np.asarray(m, dtype=bool), names[int(c.type().id())]))
    return out


def _merge(G, tables, key_cols, orders, null_orders, stream=None):
    from cudf_amd import merge as M
    o, no = _enums(orders, null_orders)
    return M.merge([_table(G, t) for t in tables], key_cols, o, no, stream=stream)


def _merge_and_check(G, tables, key_cols, orders, null_orders, id_col=None):
    from cudf_amd import sorting
    out = _merge(G, tables, key_cols, orders, null_orders)
    host = _host(out)
    R.merge_check(tables, key_cols, orders, null_orders, host, id_col=id_col)
    import cudf_amd
    o, no = _enums(orders, null_orders)
    assert sorting.is_sorted(cudf_amd.Table([out.columns()[k] for k in key_cols]), o, no)
    for c in range(len(host)):  # a column of the result is nullable if it is in an input that has rows
        assert (host[c].valid is not None) == any(t[c].valid is not None for t in tables if t[0].size), c
    return host


# ---------------------------------------------------------------- golden vectors
@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: c["name"])
def test_golden(G, c):
    for ty in c["for"]:
        tables = [S.golden_table(t, ty) for t in c["tables"]] * c.get("copies", 1)
        host = _merge_and_check(G, tables, c["key_cols"], c["orders"], c["null_orders"])
        for g, w in zip(host, S.golden_table(c["expect"], ty)):
            (gv, gm), (wv, wm) = S._rows(g), S._rows(w)
            assert np.array_equal(gm, wm) and np.array_equal(np.asarray(gv)[gm], np.asarray(wv)[wm]), ty


@pytest.mark.parametrize("order,null_order", itertools.product(GOLD["generated"][0]["orders"], GOLD["generated"][0]["null_orders"]))
def test_golden_keys_with_nulls(G, order, null_order):
    from oracle.oracle import HostColumn
    g = GOLD["generated"][0]
    n = g["rows"]
    data = np.arange(n, dtype=np.int32)
    cols = [[HostColumn(data, data % m != 0)] for m in g["nulls_at_multiples_of"]]
    tables = [R.sort_table(c, [0], [order], [null_order]) for c in cols]
    host = _merge_and_check(G, tables, [0], [order], [null_order])
    want = R.sort_table([HostColumn(np.concatenate([data, data]), np.concatenate([data % m != 0 for m in g["nulls_at_multiples_of"]]))],
                        [0], [order], [null_order])
    (gv, gm), (wv, wm) = S._rows(host[0]), S._rows(want[0])
    assert np.array_equal(gm, wm) and np.array_equal(np.asarray(gv)[gm], np.asarray(wv)[wm])


# ---------------------------------------------------------------- two random sorted tables
def _with_ids(tables, key_cols, orders, null_orders):
    """Each table sorted on its keys, then given its payload column `table_id << 32 | row` as the last column."""
    out = []
    for i, t in enumerate(tables):
        s = R.sort_table(t, key_cols, orders, null_orders)
        out.append(s + [R.payload_column(i, s[0].size)])
    return out


@functools.lru_cache(maxsize=None)
def _two_tables(na, nb):
    """(int32 key, float64 payload, int8 key): keys [2, 0] from a universe of 6; the keys are nullable in table 0 only, the payload
    in table 1 only."""
    rng = np.random.default_rng(1000 * na + nb)
    key_cols, orders, null_orders = [2, 0], ["desc", "asc"], ["after", "before"]
    make = lambda n, keys_null, pay_null: [_rand_col(rng, "int32", n, keys_null), _rand_col(rng, "float64", n, pay_null, universe=10**6),
                                           _rand_col(rng, "int8", n, keys_null)]
    tables = _with_ids([make(na, True, False), make(nb, False, True)], key_cols, orders, null_orders)
    return tables, key_cols, orders, null_orders


@pytest.mark.parametrize("na,nb", SIZES, ids=lambda x: str(x))
def test_two_random_tables(G, na, nb):
    tables, key_cols, orders, null_orders = _two_tables(na, nb)
    _merge_and_check(G, tables, key_cols, orders, null_orders, id_col=3)
    _merge_and_check(G, tables[::-1], key_cols, orders, null_orders)  # the table without key masks as the left one


def test_masks_on_one_side_only(G):
    """The nullable side is the smaller (left) table and then the larger (right) one: the output mask is right from a side without one."""
    from oracle.oracle import HostColumn
    rng = np.random.default_rng(3)
    for na, nb in ((100, 300), (300, 100)):
        a = [_rand_col(rng, "int64", na, True), _rand_col(rng, "float32", na, True)]
        b = [_rand_col(rng, "int64", nb, False), _rand_col(rng, "float32", nb, False)]
        tables = _with_ids([a, b], [0], ["asc"], ["after"])
        host = _merge_and_check(G, tables, [0], ["asc"], ["after"], id_col=2)
        assert host[0].null_count == tables[0][0].null_count and host[1].null_count == tables[0][1].null_count
        assert host[2].valid is None
    # a mask without nulls on one side, none on the other: nullable output, no nulls
    a = [HostColumn(np.arange(0, 200, 2, dtype=np.int32), np.ones(100, dtype=bool))]
    b = [HostColumn(np.arange(1, 201, 2, dtype=np.int32))]
    host = _merge_and_check(G, [a, b], [0], ["asc"], [])
    assert host[0].valid is not None and host[0].null_count == 0 and np.array_equal(np.asarray(host[0].data), np.arange(200))


# ---------------------------------------------------------------- N-way, the shortcuts
@pytest.mark.parametrize("sizes", [(5, 0, 300), (64, 1, 0, 1000), (7, 0, 130, 65, 0, 1, 2000)], ids=lambda s: f"{len(s)}_tables")
def test_n_way(G, sizes):
    rng = np.random.default_rng(len(sizes))
    raw = [[_rand_col(rng, "int16", n, True), _rand_col(rng, "uint64", n, False)] for n in sizes]
    tables = _with_ids(raw, [0, 1], ["asc", "desc"], ["before", "before"])
    host, k = _kernels_of(lambda: _merge_and_check(G, tables, [0, 1], ["asc", "desc"], ["before", "before"], id_col=2))
    rounds = sum(1 for n in sizes if n) - 1
    assert k.get("merge_positions") == 2 * rounds and k.get("merge_gather") == rounds and k.get("merge_mask") == rounds, k
    assert not k.get("sort_pack_words") and not k.get("sort_scatter") and not k.get("gather"), k


def test_one_table_no_tables_and_empty_tables(G):
    import cudf_amd
    from cudf_amd import merge as M
    from cudf_amd.types import Order
    rng = np.random.default_rng(4)
    raw = lambda n: [_rand_col(rng, "int32", n, True), _rand_col(rng, "float64", n, False)]
    empty, t, _ = tables = _with_ids([raw(0), raw(100), raw(0)], [0], ["asc"], [])
    out, k = _kernels_of(lambda: _merge_and_check(G, tables, [0], ["asc"], [], id_col=2))  # one non-empty table: a copy
    assert not k.get("merge_positions") and not k.get("merge_gather"), k
    _merge_and_check(G, [t], [0], ["asc"], [])
    out = _merge(G, [empty, empty], [0], ["asc"], [])
    assert out.num_rows() == 0 and [c.type().id().name for c in out.columns()] == ["INT32", "FLOAT64", "INT64"]
    none = M.merge([], [0], [Order.ASCENDING])
    assert isinstance(none, cudf_amd.Table) and none.num_columns() == 0


# ---------------------------------------------------------------- rejected inputs
@pytest.mark.parametrize("e", GOLD["errors"], ids=lambda e: e["name"])
def test_rejected_inputs(G, e):
    from oracle.oracle import NP_OF_TYPE_ID, TYPE_ID, HostColumn
    assert e["raises"] == "logic_error"
    tables = [[HostColumn(np.arange(rows).astype(NP_OF_TYPE_ID[TYPE_ID[ty]]), None, ty) for ty in types] for types, rows in e["tables"]]
    with pytest.raises(_lib_error()) as err:
        _merge(G, tables, e["key_cols"], e["orders"], e["null_orders"])
    assert not isinstance(err.value, (ValueError, TypeError, IndexError, MemoryError))  # the logic-error status


def test_rejected_key_tables_beyond_the_limits(G):
    from oracle.oracle import HostColumn
    wide = [HostColumn(np.arange(4, dtype=np.int32)) for _ in range(17)]
    with pytest.raises(_lib_error()):
        _merge(G, [wide, wide], list(range(17)), ["asc"] * 17, [])
    host = _merge_and_check(G, [wide, wide], [16], ["asc"], [])  # 17 columns, one of them the key: served
    assert len(host) == 17


# ---------------------------------------------------------------- 2 x 2M rows
def test_2m_rows_each(G):
    import torch

    import cudf_amd
    from cudf_amd import merge as M
    from cudf_amd import sorting
    from cudf_amd.types import Order
    n = 2 * 1024 * 1024
    gen = torch.Generator(device="cuda").manual_seed(6)
    keys = [torch.sort(torch.randint(-2**30, 2**30, (n,), device="cuda", dtype=torch.int64, generator=gen)).values for _ in range(2)]
    ids = [torch.arange(n, device="cuda", dtype=torch.int64) + (i << 32) for i in range(2)]
    tables = [cudf_amd.Table([cudf_amd.Column.from_torch(k), cudf_amd.Column.from_torch(p)]) for k, p in zip(keys, ids)]
    out = M.merge(tables, [0], [Order.ASCENDING])
    got_keys, got_ids = out.columns()[0].to_torch(), out.columns()[1].to_torch()
    assert torch.equal(got_keys, torch.sort(torch.cat(keys)).values)
    assert sorting.is_sorted(cudf_amd.Table([out.columns()[0]]), [Order.ASCENDING], [])
    for i in range(2):  # every row of each table once, in input order, with its own key
        mine = got_ids[(got_ids >> 32) == i] & 0xFFFFFFFF
        assert torch.equal(mine, torch.arange(n, device="cuda", dtype=torch.int64))
        assert torch.equal(got_keys[(got_ids >> 32) == i], keys[i])
    torch.cuda.synchronize()
