"""GPU tests of cudf::apply_boolean_mask, apply_deletion_mask, drop_nulls, drop_nans, unique and unique_count through the C ABI:
the golden vectors (tests/golden/kat_stream_compaction.json, kat_unique_count.json), seeded random tables of every column type
against the numpy restatement (tests/copy_if_restatement.py) at the row counts and selections where the kernels change path, each
also sliced, the kernels that ran, a 40M-row table that makes a wave carry its position over several rounds, a second stream and
the rejected inputs."""
import ctypes as C

import numpy as np
import pytest

import copy_if_restatement as R
from oracle.oracle import HostColumn

pytestmark = pytest.mark.gpu

GOLD = R.load_golden()
SC_GOLD = GOLD["stream_compaction"]
SELECTS = {"copy_if_select_bool", "copy_if_select_valid_words", "copy_if_select_valid_count", "copy_if_select_nan",
           "copy_if_select_unique", "copy_if_select_unique_column"}


@pytest.fixture(scope="module")
def G(gpu):
    import gpu_backend
    return gpu_backend


def _table(G, cols):
    import cudf_amd
    return cudf_amd.Table([G.to_device(c) for c in cols])


def _kernels_of(fn):
    from cudf_amd import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
    finally:
        _lib.profile_enable(False)
    return out, {k: v[0] for k, v in _lib.profile_report().items()}


def _ran(k, *names):
    """Exactly `names` of the selection kernels ran, once each."""
    assert {s: k.get(s, 0) for s in SELECTS} == {s: (1 if s in names else 0) for s in SELECTS}, k


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.itemsize])


def _mask_words(col):
    from cudf_amd import _lib
    from cudf_amd.column import _stream_ptr
    nwords = (col.offset() + col.size() + 31) // 32
    words = np.empty(nwords, dtype=np.uint32)
    sp = _stream_ptr(col.stream())
    _lib.check(_lib.load().cudf_amd_memcpy(words.ctypes.data, C.c_void_p(col.null_mask_ptr()), nwords * 4, 1, sp))
    _lib.check(_lib.load().cudf_amd_stream_synchronize(sp))
    return words


def _check(out, cols, idx):
    """`out` is the rows idx of cols: size, type, values (bit-exact where valid), validity, null_count, a mask exactly where the
    input has one, and no bit set beyond the output size."""
    got = out.columns()
    assert len(got) == len(cols)
    for g, c in zip(got, cols):
        assert g.size() == len(idx)
        assert int(g.type().id()) == c.type_id and g.type().scale() == getattr(c, "scale", 0)
        if len(idx) == 0:
            assert g.null_count() == 0
            continue
        gv, gm = g.to_numpy()
        hv, hm = R.values(c)[idx], R.valid(c)[idx]
        assert (gm is not None) == (c.valid is not None)
        assert g.nullable() == (c.valid is not None)
        if gm is not None:
            assert np.array_equal(gm, hm)
            assert g.offset() == 0
            words = _mask_words(g)
            if len(idx) % 32:
                assert int(words[-1]) >> (len(idx) % 32) == 0
        assert g.null_count() == int((~hm).sum())
        gb = _bits(np.asarray(gv).astype(np.uint8) if np.asarray(gv).dtype == np.bool_ else gv)
        assert np.array_equal(gb[hm], _bits(hv)[hm])


TYPES = [("int8", True), ("int16", False), ("int32", True), ("int64", False), ("float32", True), ("float64", True), ("bool", True),
         ("decimal64", False)]
OFFSETS = [1, 3, 33, 7, 31, 45, 13, 65]  # (none 0, none a multiple of 32)


def _rand_col(rng, ty, n, nullable, offset=0, null_p=0.3):
    total = n + offset
    npt = {"int8": np.int8, "int16": np.int16, "int32": np.int32, "int64": np.int64, "float32": np.float32,
           "float64": np.float64, "bool": np.uint8, "decimal64": np.int64}[ty]
    if ty == "bool":
        data = rng.integers(0, 2, total).astype(np.uint8)
    elif ty.startswith("float"):
        data = rng.standard_normal(total).astype(npt)
        data[rng.random(total) < 0.05] = np.nan
        data[rng.random(total) < 0.05] = -0.0
    else:
        info = np.iinfo(npt)
        data = rng.integers(info.min, info.max, total, dtype=npt, endpoint=True)
    valid = (rng.random(total) >= null_p) if nullable else None
    c = HostColumn(data, valid, ty, offset=offset)
    c.scale = -3 if ty == "decimal64" else 0
    return c


def _rand_table(rng, n, sliced):
    return [_rand_col(rng, ty, n, nullable, OFFSETS[i] if sliced else 0) for i, (ty, nullable) in enumerate(TYPES)]


def _bool_col(sel, valid=None, offset=0):
    """A BOOL8 column whose rows are `sel` (and validity `valid`), behind `offset` rows of the opposite."""
    data = np.concatenate([np.ones(offset, dtype=np.uint8), np.asarray(sel, dtype=np.uint8)])
    v = None if valid is None else np.concatenate([np.ones(offset, dtype=bool), np.asarray(valid, dtype=bool)])
    return HostColumn(data, v, "bool", offset=offset)


# ---------------------------------------------------------------- golden vectors
CASES = [(k, c) for k in ("apply_boolean_mask", "apply_deletion_mask", "drop_nulls", "drop_nans", "unique") for c in SC_GOLD[k]]


def _mirror(G):
    from cudf_amd import stream_compaction as SC
    from cudf_amd.types import DuplicateKeepOption, NullEquality
    return {
        "apply_boolean_mask": lambda cols, m: SC.apply_boolean_mask(_table(G, cols), G.to_device(m)),
        "apply_deletion_mask": lambda cols, m: SC.apply_deletion_mask(_table(G, cols), G.to_device(m)),
        "drop_nulls": lambda cols, keys, thr: SC.drop_nulls(_table(G, cols), keys, thr),
        "drop_nans": lambda cols, keys, thr: SC.drop_nans(_table(G, cols), keys, thr),
        "unique": lambda cols, keys, keep, ne: SC.unique(_table(G, cols), keys, DuplicateKeepOption["KEEP_" + keep.upper()],
                                                         NullEquality.EQUAL if ne else NullEquality.UNEQUAL),
    }


@pytest.mark.parametrize("kind,c", CASES, ids=lambda x: x if isinstance(x, str) else x["name"])
def test_golden(G, kind, c):
    cols, call = R.run_case(kind, c, _mirror(G))
    if "throws" in c:
        with pytest.raises(RuntimeError):
            call()
        return
    out = call()
    R.check_expected([col.to_numpy() for col in out.columns()], c["expect"])
    for g, ty in zip(out.columns(), c["input"]["types"]):
        assert g.type().id().name.lower().replace("bool8", "bool") == ty
        assert g.null_count() == (0 if g.to_numpy()[1] is None else int((~g.to_numpy()[1]).sum()))


@pytest.mark.parametrize("c", GOLD["unique_count"]["unique_count"], ids=lambda c: c["name"])
def test_golden_unique_count(G, c):
    from cudf_amd import reduce
    from cudf_amd.types import NanPolicy, NullEquality, NullPolicy
    cols = R.host_table(c["input"])
    if c["kind"] == "table":
        got = reduce.unique_count_table(_table(G, cols), NullEquality.EQUAL if c["nulls"] == "equal" else NullEquality.UNEQUAL)
    else:
        got = reduce.unique_count(G.to_device(cols[0]), NullPolicy[c["null_policy"].upper()], NanPolicy[c["nan_policy"].upper()])
    assert got == c["expect"]


def test_correct_null_count_rule(G):
    """ApplyBooleanMask.CorrectNullCount: a mask of all valid bits, every 277th row kept."""
    from cudf_amd import stream_compaction as SC
    n = next(g["rows"] for g in SC_GOLD["generated"] if g["name"].endswith("CorrectNullCount"))
    col = HostColumn(np.arange(n, dtype=np.int64), np.ones(n, dtype=bool))
    sel = np.arange(n) % 277 == 0
    out, k = _kernels_of(lambda: SC.apply_boolean_mask(_table(G, [col]), G.to_device(_bool_col(sel))))
    _check(out, [col], np.flatnonzero(sel))
    _ran(k, "copy_if_select_bool")
    assert k.get("copy_if_data") == 1 and k.get("copy_if_validity") == 1


def test_drop_nulls_large_column_rule(G):
    """DropNullsTest.LargeColumn at 10,000 rows: a nullable key next to a column without a mask."""
    from cudf_amd import stream_compaction as SC
    n = 10_000
    index = HostColumn(np.arange(n, dtype=np.int64))
    data = ((np.arange(n) + 1) % 3).astype(np.int32)
    cols = [index, HostColumn(data, data != 0)]
    out, k = _kernels_of(lambda: SC.drop_nulls(_table(G, cols), [1]))
    expect = np.flatnonzero((np.arange(n) - 2) % 3 != 0)
    assert expect.tolist() == R.drop_nulls(cols, [1]).tolist()
    _check(out, cols, expect)
    assert out.columns()[1].null_count() == 0 and out.columns()[1].to_numpy()[1].all()
    _ran(k, "copy_if_select_valid_words")


# ---------------------------------------------------------------- random tables at the kernels' edges
def _selections(rng, n):
    z = np.zeros(n, dtype=bool)
    out = {"none": z.copy(), "all": ~z}
    for name, pos in (("first", 0), ("last", n - 1), ("at64", 64), ("at63", 63)):
        if 0 <= pos < n:
            s = z.copy()
            s[pos] = True
            out[name] = s
    r = np.arange(n)
    out["alternating"] = r % 2 == 0
    out["period32"] = r % 32 != 5
    out["period33"] = r % 33 != 5
    for p in (0.001, 0.5, 0.999):
        out[f"bernoulli{p}"] = rng.random(n) < p
    return out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 8191, 65_537, 70_001])
def test_random_tables_at_the_edges(G, n):
    from cudf_amd import stream_compaction as SC
    rng = np.random.default_rng(n)
    for sliced in (False, True):
        cols = _rand_table(rng, n, sliced)
        t = _table(G, cols)
        for name, sel in _selections(rng, n).items():
            mvalid = (rng.random(n) < 0.9) if name.startswith("bernoulli") else None
            m = _bool_col(sel, mvalid, 37 if sliced else 0)
            out, k = _kernels_of(lambda: SC.apply_boolean_mask(t, G.to_device(m)))
            idx = R.apply_boolean_mask(cols, m)
            assert idx.tolist() == np.flatnonzero(sel & (True if mvalid is None else mvalid)).tolist()
            _check(out, cols, idx)
            if n:
                _ran(k, "copy_if_select_bool")
                assert k.get("copy_if_data", 0) == (2 if len(idx) else 0), (name, k)  # 8 columns, 4 per launch
                assert k.get("copy_if_validity", 0) == (1 if len(idx) else 0), (name, k)
                assert not k.get("gather") and not k.get("fjoin_compact"), k  # no index vector
            out = SC.apply_deletion_mask(t, G.to_device(m))
            _check(out, cols, R.apply_deletion_mask(cols, m))


def test_more_nullable_columns_than_a_validity_batch(G):
    from cudf_amd import stream_compaction as SC
    rng = np.random.default_rng(5)
    n = 5000
    cols = [_rand_col(rng, "int16", n, True, offset=i + 1) for i in range(19)]
    sel = rng.random(n) < 0.4
    out, k = _kernels_of(lambda: SC.apply_boolean_mask(_table(G, cols), G.to_device(_bool_col(sel))))
    _check(out, cols, np.flatnonzero(sel))
    assert k.get("copy_if_data") == 5 and k.get("copy_if_validity") == 2, k


# ---------------------------------------------------------------- drop_nulls
@pytest.mark.parametrize("n", [65, 4097, 70_001])
@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "sliced"])
def test_drop_nulls(G, n, sliced):
    from cudf_amd import stream_compaction as SC
    rng = np.random.default_rng(n + sliced)
    off = (lambda i: OFFSETS[i]) if sliced else (lambda i: 0)
    cols = [_rand_col(rng, "int32", n, True, off(0), 0.2), _rand_col(rng, "float64", n, True, off(1), 0.5),
            _rand_col(rng, "int64", n, False, off(2)), _rand_col(rng, "int8", n, True, off(3), 0.1),
            _rand_col(rng, "float32", n, True, off(4), 0.0)]  # (3: payload; 4: a mask without a null)
    t = _table(G, cols)
    keys = [0, 1, 2]

    def run(keys, thr):
        out, k = _kernels_of(lambda: SC.drop_nulls(t, keys, thr))
        _check(out, cols, R.drop_nulls(cols, keys, thr))
        return out, k

    # every key: the word-wise kernel, never the counting one
    out, k = run(keys, None)
    _ran(k, "copy_if_select_valid_words")
    assert out.num_rows() == int((R.valid(cols[0]) & R.valid(cols[1])).sum())  # the mask-less key counts as valid
    out, k = run(keys, 3)
    _ran(k, "copy_if_select_valid_words")
    # a mid threshold: one of the two nullable keys (the mask-less key gives the other)
    out, k = run(keys, 2)
    _ran(k, "copy_if_select_valid_count")
    assert out.num_rows() == int((R.valid(cols[0]) | R.valid(cols[1])).sum())
    # the mask-less key meets it alone: every row, no kernel; nothing can meet it: no row, no kernel
    for thr, rows in ((1, n), (0, n), (4, 0)):
        out, k = run(keys, thr)
        _ran(k)
        assert out.num_rows() == rows and not k.get("copy_if_data"), k
    # no key has a null: a copy, whatever the threshold
    for ks in ([2], [4], [2, 4]):
        out, k = run(ks, 5)
        _ran(k)
        assert out.num_rows() == n
    out, k = run([], None)
    assert out.num_rows() == n
    # one nullable key among sixteen
    out, k = run([1] + [2] * 15, None)
    _ran(k, "copy_if_select_valid_words")


# ---------------------------------------------------------------- drop_nans
@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "sliced"])
def test_drop_nans(G, sliced):
    from cudf_amd import stream_compaction as SC
    rng = np.random.default_rng(17 + sliced)
    n = 70_001
    f32 = _rand_col(rng, "float32", n, True, 5 if sliced else 0)
    f64 = _rand_col(rng, "float64", n, False, 33 if sliced else 0)
    # both NaN signs and payloads; NaNs under null bits
    b32, b64 = _bits(f32.data), _bits(f64.data)
    r = rng.random(len(b32))
    b32[r < 0.05] = 0xFFC00001
    b32[(r >= 0.05) & (r < 0.1)] = 0x7F800001
    r = rng.random(len(b64))
    b64[r < 0.05] = 0xFFF8000000000123
    b64[(r >= 0.05) & (r < 0.1)] = 0x7FF0000000000001
    assert (np.isnan(R.values(f32)) & ~R.valid(f32)).any()
    cols = [f32, _rand_col(rng, "int32", n, True, 7 if sliced else 0), f64]
    t = _table(G, cols)
    for keys, thr in (([0, 2], None), ([0, 2], 1), ([0], None), ([2], 1), ([2, 0], 2), ([0, 2], 0), ([0, 2], 3)):
        out, k = _kernels_of(lambda: SC.drop_nans(t, keys, thr))
        _check(out, cols, R.drop_nans(cols, keys, thr))
        _ran(k, "copy_if_select_nan")
    assert SC.drop_nans(t, []).num_rows() == n
    nn32, nn64 = ~np.isnan(R.values(f32)) | ~R.valid(f32), ~np.isnan(R.values(f64))
    assert SC.drop_nans(t, [0, 2]).num_rows() == int((nn32 & nn64).sum())


# ---------------------------------------------------------------- unique / unique_count
def _runs_table(rng, n, sliced):
    """Two key columns (float64 with NaN, +-0 and nulls; int32) in runs of length 1, 2, 64, 65 and 4097, one of them across rows
    4095 | 4096 and one across 8191 | 8192, and a payload column."""
    lengths = [1, 2, 64, 65, 4097]  # the last covers rows 132 .. 4228
    lengths += [1] * (8191 - sum(lengths)) + [2]  # rows 8191 | 8192
    while sum(lengths) < n:
        lengths.append(int(rng.choice([1, 1, 2, 3, 64, 65, 700])))
    run = np.repeat(np.arange(len(lengths)), lengths)[:n]
    palette = np.array([1.5, np.nan, 0.0, 7.0, np.nan, -3.25, 0.0])
    k0 = palette[run % len(palette)]
    flip = rng.random(n) < 0.5
    k0 = np.where((k0 == 0) & flip, -0.0, k0)  # -0 equals +0 inside a run
    b = _bits(k0)
    b[np.isnan(k0) & flip] = 0xFFF8000000000042  # another NaN equals NaN
    v0 = (run % 5) != 3  # whole runs of nulls
    k1 = (run % 3).astype(np.int32)
    off = [3, 33, 7] if sliced else [0, 0, 0]

    def col(data, valid, ty, o):
        pad = np.zeros(o, dtype=data.dtype)
        return HostColumn(np.concatenate([pad, data]), None if valid is None else np.concatenate([np.ones(o, dtype=bool), valid]), ty, offset=o)
    return [col(rng.integers(0, 1000, n).astype(np.int64), rng.random(n) < 0.7, "int64", off[0]), col(k0, v0, "float64", off[1]),
            col(k1, None, "int32", off[2])]


@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "sliced"])
def test_unique_and_unique_count(G, sliced):
    from cudf_amd import reduce
    from cudf_amd import stream_compaction as SC
    from cudf_amd.types import DuplicateKeepOption, NanPolicy, NullEquality, NullPolicy
    rng = np.random.default_rng(23 + sliced)
    n = 70_001
    cols = _runs_table(rng, n, sliced)
    t = _table(G, cols)
    kt = _table(G, cols[1:])
    for ne in (True, False):
        eq = NullEquality.EQUAL if ne else NullEquality.UNEQUAL
        for keep in ("any", "first", "last", "none"):
            out, k = _kernels_of(lambda: SC.unique(t, [1, 2], DuplicateKeepOption["KEEP_" + keep.upper()], eq))
            idx = R.unique(cols, [1, 2], keep, ne)
            _check(out, cols, idx)
            _ran(k, "copy_if_select_unique")
            if ne and keep in ("first", "last"):  # the long run keeps one row, across the chunk boundary
                assert ((idx >= 132) & (idx <= 4228)).sum() == 1 and (8191 if keep == "first" else 8192) in idx
        got, k = _kernels_of(lambda: reduce.unique_count_table(kt, eq))
        assert got == R.unique_count_table(cols[1:], ne) == len(R.unique(cols, [1, 2], "first", ne))
        _ran(k, "copy_if_select_unique")
        assert not k.get("copy_if_data") and not k.get("copy_if_validity"), k
    for c in (cols[1], cols[2], cols[0]):
        d = G.to_device(c)
        for include in (True, False):
            for nan_is_null in (True, False):
                got, k = _kernels_of(lambda: reduce.unique_count(d, NullPolicy.INCLUDE if include else NullPolicy.EXCLUDE,
                                                                 NanPolicy.NAN_IS_NULL if nan_is_null else NanPolicy.NAN_IS_VALID))
                assert got == R.unique_count_column(c, include, nan_is_null), (include, nan_is_null)
                _ran(k, "copy_if_select_unique_column")
                assert not k.get("copy_if_data") and not k.get("copy_if_validity"), k
    assert SC.unique_count is reduce.unique_count


def test_unique_small_runs(G):
    """Row counts below one chunk, every keep: the first and the last row have one neighbour only."""
    from cudf_amd import stream_compaction as SC
    from cudf_amd.types import DuplicateKeepOption
    for n, key in ((1, [4]), (2, [4, 4]), (2, [4, 5]), (65, [1] * 64 + [2]), (66, [0] + [1] * 65)):
        cols = [HostColumn(np.arange(n, dtype=np.int16), np.arange(n) % 3 != 0), HostColumn(np.array(key, dtype=np.int8))]
        for keep in ("any", "first", "last", "none"):
            out = SC.unique(_table(G, cols), [1], DuplicateKeepOption["KEEP_" + keep.upper()])
            _check(out, cols, R.unique(cols, [1], keep))


# ---------------------------------------------------------------- a chunk of more than 64 words
def test_forty_million_rows_carry_the_position_across_rounds(G):
    """Beyond 8192 x 4096 rows a chunk holds more than 64 selection words: a wave loops and carries its position."""
    from cudf_amd import stream_compaction as SC
    n = 40_000_003
    rng = np.random.default_rng(40)
    a = rng.integers(-2**31, 2**31, n, dtype=np.int64).astype(np.int32)
    va = np.unpackbits(np.frombuffer(rng.bytes((n + 7) // 8), dtype=np.uint8))[:n].astype(bool)
    b = rng.random(n)
    sel = np.unpackbits(np.frombuffer(rng.bytes((n + 7) // 8), dtype=np.uint8))[:n].astype(bool)
    cols = [HostColumn(a, va), HostColumn(b)]
    out, k = _kernels_of(lambda: SC.apply_boolean_mask(_table(G, cols), G.to_device(HostColumn(sel.view(np.uint8), None, "bool"))))
    ga, gva = out.columns()[0].to_numpy()
    gb, gvb = out.columns()[1].to_numpy()
    assert gvb is None and np.array_equal(gb, b[sel])
    assert np.array_equal(gva, va[sel]) and np.array_equal(ga[gva], a[sel][gva])
    assert out.columns()[0].null_count() == int((~va[sel]).sum())
    assert k.get("copy_if_validity") == 1 and k.get("copy_if_data") == 1, k


# ---------------------------------------------------------------- streams, rejected inputs
def test_non_default_stream(G):
    import torch

    from cudf_amd import reduce
    from cudf_amd import stream_compaction as SC
    from cudf_amd.types import DuplicateKeepOption
    rng = np.random.default_rng(11)
    n = 300_000
    cols = _rand_table(rng, n, True)
    sel = rng.random(n) < 0.5
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = _table(G, cols)
        out = SC.apply_boolean_mask(t, G.to_device(_bool_col(sel)), stream=s)
        dropped = SC.drop_nulls(t, [0, 2], stream=s)
        uniq = SC.unique(t, [6], DuplicateKeepOption.KEEP_FIRST, stream=s)
        count = reduce.unique_count_table(_table(G, [cols[6]]), stream=s)
    s.synchronize()
    _check(out, cols, np.flatnonzero(sel))
    _check(dropped, cols, R.drop_nulls(cols, [0, 2]))
    _check(uniq, cols, R.unique(cols, [6], "first"))
    assert count == uniq.num_rows()


def test_rejected_inputs(G):
    from cudf_amd import _lib
    from cudf_amd import stream_compaction as SC
    from cudf_amd.types import DuplicateKeepOption
    cols = [HostColumn(np.arange(10, dtype=np.int32)), HostColumn(np.arange(10, dtype=np.float64))]
    t = _table(G, cols)
    with pytest.raises(RuntimeError):  # size mismatch
        SC.apply_boolean_mask(t, G.to_device(_bool_col(np.ones(9))))
    with pytest.raises(RuntimeError):
        SC.apply_deletion_mask(t, G.to_device(_bool_col(np.ones(11))))
    with pytest.raises(RuntimeError):  # not BOOL8
        SC.apply_boolean_mask(t, G.to_device(HostColumn(np.ones(10, dtype=np.int8))))
    assert SC.apply_boolean_mask(t, G.to_device(_bool_col(np.ones(0)))).num_rows() == 0  # an empty mask: an empty table
    with pytest.raises(RuntimeError):  # a key that is not floating point
        SC.drop_nans(t, [1, 0])
    for fn in (SC.drop_nulls, SC.drop_nans, lambda t, k: SC.unique(t, k, DuplicateKeepOption.KEEP_FIRST)):
        with pytest.raises(IndexError):
            fn(t, [0, 2])
        with pytest.raises(IndexError):
            fn(t, [-1])
    wide_cols = [HostColumn(np.arange(10, dtype=np.float64), np.arange(10) % 2 == 0) for _ in range(17)]
    wide = _table(G, wide_cols)
    for fn in (SC.drop_nulls, SC.drop_nans, lambda t, k: SC.unique(t, k, DuplicateKeepOption.KEEP_FIRST)):
        with pytest.raises(RuntimeError):
            fn(wide, list(range(17)))
    _check(SC.drop_nulls(wide, list(range(16))), wide_cols, np.arange(0, 10, 2))  # sixteen keys and a payload column pass
    out, keys = C.c_void_p(), (C.c_int32 * 1)(0)
    for ncols, nkeys in ((2, -1), (-1, 1)):  # negative counts: rejected before any range is formed
        assert _lib.load().cudf_amd_drop_nulls(t._views(), ncols, keys, nkeys, -1, None, C.byref(out)) == 2
        assert _lib.load().cudf_amd_unique(t._views(), ncols, keys, nkeys, 1, 1, None, C.byref(out)) == 2
