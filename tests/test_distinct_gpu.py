"""GPU tests of cudf::distinct, distinct_indices, stable_distinct and distinct_count through the C ABI: the golden vectors
(tests/golden/kat_distinct.json), seeded random tables against the numpy restatement (tests/distinct_restatement.py) over every
keep x null_equality x nan_equality with each form forced through the CUDF_AMD_DISTINCT_* settings and proven by the kernels that
ran, payload and sliced columns, a second stream, the rejected inputs, and a 100M-row property against torch.unique."""
import numpy as np
import pytest

import distinct_restatement as R

pytestmark = pytest.mark.gpu

GOLD = R.load_golden()
KEEPS = ["any", "first", "last", "none"]
FORMS = {  # form -> (settings, the build kernel that must run)
    "dense_lds": ({}, "distinct_dense_lds_build"),
    "dense": ({"CUDF_AMD_DISTINCT_LDS_ENTRIES": "0"}, "distinct_dense_build"),
    "set_inline": ({"CUDF_AMD_DISTINCT_DENSE": "0"}, "distinct_set_build_inline"),
    "set_rows": ({"CUDF_AMD_DISTINCT_DENSE": "0", "CUDF_AMD_DISTINCT_INLINE": "0"}, "distinct_set_build_rows"),
}
BUILDS = {b for _, b in FORMS.values()}


@pytest.fixture(scope="module")
def G(gpu):
    import gpu_backend
    return gpu_backend


def _table(G, cols):
    import cudf_amd
    return cudf_amd.Table([G.to_device(c) for c in cols])


def _keep(k):
    from cudf_amd.types import DuplicateKeepOption
    return DuplicateKeepOption["KEEP_" + k.upper()]


def _eqs(nulls_equal, nans_equal):
    from cudf_amd.types import NanEquality, NullEquality
    return (NullEquality.EQUAL if nulls_equal else NullEquality.UNEQUAL, NanEquality.ALL_EQUAL if nans_equal else NanEquality.UNEQUAL)


def _indices(col):
    assert col.type().id().name == "INT32" and col.null_count() == 0
    return col.to_numpy()[0]


def _kernels_of(fn):
    from cudf_amd import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
    finally:
        _lib.profile_enable(False)
    return out, {k: v[0] for k, v in _lib.profile_report().items()}


def _rows_of(col):
    """Device column -> (values, valid) on the host."""
    data, valid = col.to_numpy()
    return np.asarray(data), (np.ones(len(data), dtype=bool) if valid is None else np.asarray(valid, dtype=bool))


def _host_rows(c):
    v = np.asarray(c.data)[c.offset:c.offset + c.size]
    valid = np.ones(c.size, dtype=bool) if c.valid is None else np.asarray(c.valid[c.offset:c.offset + c.size], dtype=bool)
    return v, valid


def _same(a, b):
    """Equal values, NaN equal to NaN, bit-exact otherwise (so that -0 and +0 stay apart: a row is copied whole)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return np.array_equal(a.view(np.uint32 if a.itemsize == 4 else np.uint64), b.view(np.uint32 if b.itemsize == 4 else np.uint64))
    return np.array_equal(a.astype(b.dtype), b)


def _check_gathered(out_table, cols, idx):
    """Every column of the result is the input's column gathered at idx (payload included)."""
    got = out_table.columns()
    assert len(got) == len(cols)
    for g, c in zip(got, cols):
        gv, gm = _rows_of(g)
        hv, hm = _host_rows(c)
        assert np.array_equal(gm, hm[idx])
        assert _same(np.where(gm, gv, 0), np.where(hm[idx], hv[idx], 0))


def _row_set(cols):
    """The rows of device columns or HostColumns as a set of tuples of (valid, value bits)."""
    parts = []
    for c in cols:
        v, m = _rows_of(c) if hasattr(c, "to_numpy") else _host_rows(c)
        v = np.asarray(v)
        bits = v.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[v.itemsize]).astype(np.uint64)
        parts.append(np.where(m, bits, 0).tolist())
        parts.append(m.tolist())
    return set(zip(*parts))


def _check_any(idx, keys, nulls_equal, nans_equal):
    """KEEP_ANY: one surviving row per set of equal rows (its own row, so it holds its key), every row that equals none kept."""
    alone, ids = R._groups(keys, nulls_equal, nans_equal)
    assert np.all(np.diff(idx.astype(np.int64)) > 0)
    chosen = ids[idx]
    assert np.array_equal(np.sort(chosen[chosen >= 0]), np.unique(ids[ids >= 0]))  # each set exactly once
    assert np.array_equal(np.flatnonzero(alone), idx[chosen < 0])


def _check_indices(idx, keys, keep, nulls_equal, nans_equal):
    if keep == "any":
        _check_any(idx, keys, nulls_equal, nans_equal)
    else:
        assert idx.tolist() == R.distinct_indices(keys, keep, nulls_equal, nans_equal).tolist()


# ---------------------------------------------------------------- golden vectors
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("c", GOLD["distinct"], ids=lambda c: c["name"])
def test_golden_distinct(G, c, stable):
    from cudf_amd import stream_compaction as SC
    cols = R.host_table(c["input"])
    ne, nan = _eqs(c["nulls"] == "equal", c["nans"] == "equal")
    fn = SC.stable_distinct if stable else SC.distinct
    out = fn(_table(G, cols), c["keys"], _keep(c["keep"]), ne, nan)
    assert out.num_columns() == len(cols)
    if not cols:
        return
    got, _ = _rows_of(out.columns()[0])
    assert sorted(got.tolist()) == c["expect_payload_sorted"]
    if "expect_indices" in c:
        _check_gathered(out, cols, np.array(c["expect_indices"], dtype=np.int64))
        if c["keys"]:
            idx = _indices(SC.distinct_indices(_table(G, [cols[k] for k in c["keys"]]), _keep(c["keep"]), ne, nan))
            assert idx.tolist() == c["expect_indices"]


@pytest.mark.parametrize("form", ["default", "set_rows"])
@pytest.mark.parametrize("c", GOLD["stable_distinct"], ids=lambda c: c["name"])
def test_golden_stable_distinct_order(G, monkeypatch, c, form):
    """stable_distinct_tests.cpp pins the row order, KEEP_ANY included: column 0 of the result, in order, on the default form and on
    {hash | row} slots."""
    from cudf_amd import stream_compaction as SC
    for k, v in (FORMS[form][0] if form != "default" else {}).items():
        monkeypatch.setenv(k, v)
    cols = R.host_table(c["input"])
    ne, nan = _eqs(c["nulls"] == "equal", c["nans"] == "equal")
    out = SC.stable_distinct(_table(G, cols), c["keys"], _keep(c["keep"]), ne, nan)
    assert out.num_columns() == len(cols)
    if not cols:
        return
    got, _ = _rows_of(out.columns()[0])
    assert got.tolist() == c["expect_payload_in_order"]


@pytest.mark.parametrize("c", GOLD["distinct_count"], ids=lambda c: c["name"])
def test_golden_distinct_count(G, c):
    from cudf_amd import reduce
    from cudf_amd.types import NanPolicy, NullEquality, NullPolicy
    cols = R.host_table(c["input"])
    if c["kind"] == "table":
        got = reduce.distinct_count_table(_table(G, cols), NullEquality.EQUAL if c["nulls"] == "equal" else NullEquality.UNEQUAL)
    else:
        got = reduce.distinct_count(_table(G, cols).columns()[0],
                                    NullPolicy.INCLUDE if c["null_policy"] == "include" else NullPolicy.EXCLUDE,
                                    NanPolicy.NAN_IS_NULL if c["nan_policy"] == "nan_is_null" else NanPolicy.NAN_IS_VALID)
    assert got == c["expect"]


# ---------------------------------------------------------------- random tables, every rule, each form
TYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "bool", "float32", "float64",
         "timestamp_ms", "decimal64"]


def _rand_col(rng, ty, n, universe, null_p, offset=0):
    from oracle.oracle import NP_OF_TYPE_ID, TYPE_ID, HostColumn
    npt = NP_OF_TYPE_ID[TYPE_ID[ty]]
    m = n + offset
    if ty == "bool":
        data = rng.random(m) < 0.5
    elif "float" in ty:
        pool = np.concatenate([[0.0, -0.0, np.nan, np.inf, -np.inf], np.arange(universe) * 0.75 - universe / 3]).astype(npt)
        data = pool[rng.integers(0, len(pool), m)]
        neg_nan = rng.random(m) < 0.02  # -NaN: the sign bit set on a NaN
        bits = data.view(np.uint32 if npt == np.float32 else np.uint64)
        bits[neg_nan] = np.array(np.nan, dtype=npt).view(bits.dtype) | (bits.dtype.type(1) << bits.dtype.type(8 * bits.itemsize - 1))
    else:
        info = np.iinfo(npt)
        lo = max(int(info.min), -(universe // 2)) if info.min < 0 else 0
        data = rng.integers(lo, min(int(info.max), lo + universe - 1), m, endpoint=True).astype(npt)
    valid = rng.random(m) >= null_p if null_p > 0 else None
    return HostColumn(data, valid, ty, offset=offset)


@pytest.mark.parametrize("ty", TYPES)
def test_random_one_key_every_rule(G, ty):
    from cudf_amd import stream_compaction as SC
    rng = np.random.default_rng(TYPES.index(ty))
    keys = [_rand_col(rng, ty, 60_000, 3000, 0.05, offset=3)]
    t = _table(G, keys)
    for keep in KEEPS:
        for ne in (True, False):
            for nan in (True, False):
                idx = _indices(SC.distinct_indices(t, _keep(keep), *_eqs(ne, nan)))
                _check_indices(idx, keys, keep, ne, nan)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("ty", ["int16", "int32", "int64", "uint64", "timestamp_ms", "decimal64"])
def test_each_form_forced(G, monkeypatch, form, ty):
    """The same rules with each form forced, proven by the build kernel that ran (and no other)."""
    from cudf_amd import reduce
    from cudf_amd import stream_compaction as SC
    env, build = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if form == "dense_lds" and ty == "int16":  # (a 2-byte key spans 2^16 words, beyond the LDS build: its 1-byte sibling)
        ty = "int8"
    if form == "set_inline" and ty == "int16":  # (only 4- and 8-byte keys sit in the slot)
        build = FORMS["set_rows"][1]
    if form == "dense_lds" and ty != "int16":
        monkeypatch.setenv("CUDF_AMD_DISTINCT_DENSE_RATIO", str(1 << 20))
    rng = np.random.default_rng(len(form) * 31 + len(ty))
    universe = 4000 if form.startswith("dense") else 200_000
    keys = [_rand_col(rng, ty, 150_000, universe, 0.05, offset=5)]
    t = _table(G, keys)
    for keep in KEEPS:
        for ne in (True, False):
            idx, k = _kernels_of(lambda: _indices(SC.distinct_indices(t, _keep(keep), *_eqs(ne, True))))
            _check_indices(idx, keys, keep, ne, True)
            assert k.get(build, 0) == 1 and k.get("distinct_sweep", 0) == 1, k
            assert not any(k.get(o, 0) for o in BUILDS - {build}), k
    n, k = _kernels_of(lambda: reduce.distinct_count_table(t))
    assert n == R.distinct_count_table(keys) and k.get(build, 0) == 1 and not k.get("distinct_sweep"), k


@pytest.mark.parametrize("form", ["set_inline", "set_rows"])
@pytest.mark.parametrize("ty", ["float32", "float64"])
def test_float_keys_each_set_form(G, monkeypatch, form, ty):
    from cudf_amd import stream_compaction as SC
    for k, v in FORMS[form][0].items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(len(form) + len(ty))
    keys = [_rand_col(rng, ty, 80_000, 500, 0.05, offset=1)]
    t = _table(G, keys)
    for keep in KEEPS:
        for ne in (True, False):
            for nan in (True, False):
                idx, k = _kernels_of(lambda: _indices(SC.distinct_indices(t, _keep(keep), *_eqs(ne, nan))))
                _check_indices(idx, keys, keep, ne, nan)
                assert k.get(FORMS[form][1], 0) == 1, k


@pytest.mark.parametrize("form", ["set_inline", "set_rows"])
@pytest.mark.parametrize("ty", ["int64", "uint64"])
def test_all_ones_key_each_set_form(G, monkeypatch, form, ty):
    """The 8-byte key whose bits are all ones (int64 -1, uint64 2^64 - 1) is the word of an empty slot: the inline set gives it a
    state word of its own; in {hash | row} slots it is a key like any other. 1,000 rows with duplicates and a few NULLs, every keep
    rule and the count."""
    from oracle.oracle import HostColumn
    from cudf_amd import reduce
    from cudf_amd import stream_compaction as SC
    env, build = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(len(form) + len(ty))
    npt = np.dtype(ty).type
    data = rng.integers(0, 300, 1000).astype(npt)
    ones_rows = [0, 5, 333, 640, 999]
    data[ones_rows] = npt(-1) if ty == "int64" else npt(2**64 - 1)
    valid = rng.random(1000) >= 0.01
    valid[ones_rows] = True
    keys = [HostColumn(data, valid, ty)]
    t = _table(G, keys)
    for keep in KEEPS:
        for ne in (True, False):
            idx, k = _kernels_of(lambda: _indices(SC.distinct_indices(t, _keep(keep), *_eqs(ne, True))))
            _check_indices(idx, keys, keep, ne, True)
            kept = set(ones_rows) & set(idx.tolist())
            assert {"any": len(kept) == 1, "first": kept == {0}, "last": kept == {999}, "none": not kept}[keep], kept
            assert k.get(build, 0) == 1 and not any(k.get(o, 0) for o in BUILDS - {build}), k
    n, k = _kernels_of(lambda: reduce.distinct_count_table(t))
    assert n == R.distinct_count_table(keys) and k.get(build, 0) == 1 and not k.get("distinct_sweep"), k


@pytest.mark.parametrize("types", [("int32", "int8"), ("int64", "float64", "bool"), ("uint16", "float32", "decimal64", "int64")],
                         ids=lambda t: "_".join(t))
def test_several_keys_with_payload(G, types):
    """1-4 key columns among payload columns, all sliced: distinct / stable_distinct gather whole rows."""
    from cudf_amd import stream_compaction as SC
    rng = np.random.default_rng(sum(map(len, types)))
    n = 50_000
    keys = [_rand_col(rng, ty, n, 6, 0.05, offset=i + 1) for i, ty in enumerate(types)]
    payload = [_rand_col(rng, "float64", n, 10**6, 0.1, offset=2), _rand_col(rng, "int32", n, 10**6, 0.0, offset=4)]
    cols = [payload[0]] + keys + [payload[1]]
    key_idx = list(range(1, 1 + len(keys)))
    t = _table(G, cols)
    for keep in KEEPS:
        for ne in (True, False):
            for nan in (True, False):
                idx = _indices(SC.distinct_indices(_table(G, keys), _keep(keep), *_eqs(ne, nan)))
                _check_indices(idx, keys, keep, ne, nan)
                for fn in (SC.distinct, SC.stable_distinct):
                    out = fn(t, key_idx, _keep(keep), *_eqs(ne, nan))
                    if keep == "any":  # (another call may pick other rows of a set: check the count, and that rows stay whole)
                        assert out.num_rows() == len(idx)
                        assert _row_set(out.columns()) <= _row_set(cols)
                    else:
                        _check_gathered(out, cols, idx.astype(np.int64))


def test_non_default_stream(G):
    import torch

    from cudf_amd import reduce
    from cudf_amd import stream_compaction as SC
    rng = np.random.default_rng(11)
    keys = [_rand_col(rng, "int64", 300_000, 50_000, 0.02)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = _table(G, keys)
        idx = SC.distinct_indices(t, _keep("first"), stream=s)
        n = reduce.distinct_count_table(t, stream=s)
    s.synchronize()
    assert _indices(idx).tolist() == R.distinct_indices(keys, "first").tolist()
    assert n == R.distinct_count_table(keys)


def test_rejected_inputs(G):
    from cudf_amd import stream_compaction as SC
    from oracle.oracle import HostColumn
    t = _table(G, [HostColumn(np.arange(10, dtype=np.int32)), HostColumn(np.arange(10, dtype=np.int64))])
    with pytest.raises(IndexError):
        SC.distinct(t, [0, 2])
    with pytest.raises(IndexError):
        SC.stable_distinct(t, [-1])
    import ctypes as C

    from cudf_amd import _lib
    out, keys = C.c_void_p(), (C.c_int32 * 1)(0)
    for ncols, nkeys in ((2, -1), (-1, 1)):  # negative counts: rejected before any range is formed
        assert _lib.load().cudf_amd_distinct(t._views(), ncols, keys, nkeys, 0, 1, 1, 0, None, C.byref(out)) == 2
    wide = _table(G, [HostColumn(np.arange(10, dtype=np.int32)) for _ in range(17)])  # beyond MAX_COLS
    with pytest.raises(RuntimeError):
        SC.distinct_indices(wide)
    with pytest.raises(RuntimeError):
        SC.distinct(wide, list(range(17)))


# ---------------------------------------------------------------- 100M rows against torch
@pytest.mark.parametrize("shape", ["dense", "sparse"])
def test_100m_rows_against_torch(G, shape):
    import torch

    import cudf_amd
    from cudf_amd import reduce
    from cudf_amd import stream_compaction as SC
    n = 100_000_000
    gen = torch.Generator(device="cuda").manual_seed(7)
    if shape == "dense":
        k = torch.randint(0, 1_000_000, (n,), device="cuda", dtype=torch.int64, generator=gen)
    else:
        pool = torch.randint(-2**62, 2**62, (50_000_000,), device="cuda", dtype=torch.int64, generator=gen)
        k = pool[torch.randint(0, 50_000_000, (n,), device="cuda", dtype=torch.int64, generator=gen)]
    t = cudf_amd.Table([cudf_amd.Column.from_torch(k)])
    uniq, inv = torch.unique(k, return_inverse=True)
    first = torch.full((uniq.numel(),), n, device="cuda", dtype=torch.int64)
    first = first.scatter_reduce(0, inv, torch.arange(n, device="cuda", dtype=torch.int64), reduce="amin")
    expect = torch.sort(first).values
    assert reduce.distinct_count_table(t) == uniq.numel()
    any_idx = SC.distinct_indices(t, _keep("any")).to_torch()
    assert any_idx.numel() == uniq.numel()
    got = SC.distinct_indices(t, _keep("first")).to_torch().to(torch.int64)
    assert torch.equal(got, expect)
    del uniq, inv, first, expect, got, any_idx
    torch.cuda.synchronize()
