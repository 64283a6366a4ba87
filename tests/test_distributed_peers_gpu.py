"""cudf::distributed (cudf_amd/csrc/distributed/) with peers beyond one non-null int64 key: the four collectives
(shuffle, shuffle_groupby, combine_groupby, shuffle_join) on loopback worlds of 2, 4 and 8 virtual ranks, checked against the CPU
oracle run on the concatenation of all shards.

Every check is threefold:
  - completeness and disjointness: every expected group / row comes back, and from exactly one rank (float keys compared as
    classes: -0.0 == +0.0, every NaN equal; null keys by validity);
  - ownership: every returned key row on rank r has (oracle.row_hash(keys) * world) >> 32 == r;
  - values: integers, counts, MIN / MAX, validity and type ids exact; float SUM / MEAN / SUM_OF_SQUARES within a per-group bound
    from the group's own inputs (kat.sum_atol in the value type's epsilon), float PRODUCT within m_g * eps relative.
"""
import collections

import numpy as np
import pytest

from loopback_world import run_ranks

gpu = pytest.mark.gpu
OFFSETS = (1, 33, 67)  # slice offsets: not multiples of 32, so validity bits start mid-word
INT_VALUE_TYPES = ("int8", "int32", "uint64", "decimal64", "timestamp_ms")


def _tname(tid):
    from oracle.oracle import TYPE_ID
    return {v: k for k, v in TYPE_ID.items()}[tid]


def _device(data, valid, tname, offset=0, scale=0):
    """Device column over the FULL host buffers, sliced at `offset` (Arrow offset semantics)."""
    import cudf_amd
    from cudf_amd.types import DataType, TypeId
    from oracle.oracle import TYPE_ID
    return cudf_amd.Column.from_numpy(data, valid, dtype=DataType(TypeId(TYPE_ID[tname]), scale), offset=offset)


def _fetch(col):
    """(data, valid or None, type id) of a device column, and its scale."""
    data, valid = col.to_numpy()
    return (data, valid, int(col.type().id())), col.type().scale()


def _cat(cols):
    """The ranks' pieces of one column, one after the other."""
    data = np.concatenate([c[0] for c in cols])
    valid = None if all(c[1] is None for c in cols) else np.concatenate(
        [np.ones(len(c[0]), bool) if c[1] is None else c[1] for c in cols])
    return data, valid, cols[0][2]


def canon_rows(cols):
    """Rows of (data, valid, type id) columns as hashable tuples: NULL -> None, floats as classes (-0.0 -> +0.0, every NaN ->
    "nan"), everything else by value."""
    from oracle.oracle import NP_OF_TYPE_ID
    per_col = []
    for data, valid, tid in cols:
        if np.dtype(NP_OF_TYPE_ID[tid]).kind == "f":
            with np.errstate(invalid="ignore"):  # (signalling NaNs)
                vals = [("nan" if x != x else x) for x in (data.astype(np.float64) + 0.0).tolist()]
        else:
            vals = data.astype(np.int64 if data.dtype != np.uint64 else np.uint64).tolist()
        if valid is not None:
            vals = [x if v else None for x, v in zip(vals, valid.tolist())]
        per_col.append(vals)
    return list(zip(*per_col)) if per_col else []


def _owners(oracle, cols, world):
    """Owner rank of every row of the key columns (data, valid, type id)."""
    from oracle.oracle import HostColumn
    h = oracle.row_hash([HostColumn(d, v, _tname(t)) for d, v, t in cols], 0).astype(np.uint64)
    return ((h * np.uint64(world)) >> np.uint64(32)).astype(np.int64)


def _check_owned(oracle, world, r, key_cols):
    if len(key_cols[0][0]):
        assert (_owners(oracle, key_cols, world) == r).all(), f"rank {r} returned a key it does not own"


def _align(got_keys, exp_keys):
    """Index array `order` with got row order[i] <-> expected row i; fails on a missing, extra or repeated group."""
    g, e = canon_rows(got_keys), canon_rows(exp_keys)
    assert len(set(e)) == len(e), "oracle returned a key twice"
    dup = [k for k, c in collections.Counter(g).items() if c > 1]
    assert not dup, f"{len(dup)} groups came back from two ranks, e.g. {dup[:4]}"
    missing, extra = set(e) - set(g), set(g) - set(e)
    assert not missing and not extra, f"missing groups {list(missing)[:4]} ({len(missing)}), extra {list(extra)[:4]} ({len(extra)})"
    pos = {k: i for i, k in enumerate(g)}
    return np.array([pos[k] for k in e], dtype=np.int64)


def _take(col, order):
    d, v, t = col
    return d[order], None if v is None else v[order], t


# ------------------------------------------------------------------ data
def _special_float(code, rank, i, dtype):
    """Float key classes: code 0 -> -0.0 on even ranks, +0.0 on odd ones; code 1 -> NaN of varying payload and sign; 2 / 3 -> +inf /
    -inf; otherwise a distinct exact value."""
    out = ((code - 700) * 0.25).astype(dtype)
    out[code == 2] = np.inf
    out[code == 3] = -np.inf
    out[code == 0] = -0.0 if rank % 2 == 0 else 0.0
    nan = np.flatnonzero(code == 1)
    if dtype == np.float64:
        bits = (np.uint64(0x7ff0000000000000) | (np.uint64(1) + (np.uint64(rank * 977) + nan.astype(np.uint64)) % np.uint64(1 << 51))
                | np.where(nan % 2 == 1, np.uint64(1 << 63), np.uint64(0)))
        out[nan] = bits.view(np.float64)
    else:
        bits = (np.uint32(0x7f800000) | (np.uint32(1) + (np.uint32(rank * 977) + nan.astype(np.uint32)) % np.uint32(1 << 22))
                | np.where(nan % 2 == 1, np.uint32(1 << 31), np.uint32(0)).astype(np.uint32))
        out[nan] = bits.astype(np.uint32).view(np.float32)
    return out


def _groupby_keys(shape, code, rank, rng, all_null=False):
    """Key columns [(data, valid, type name)] of one rank for a key shape, from each row's group code."""
    n = len(code)
    if shape == "int64":
        return [((code - 700) * 1_000_003, None, "int64")]
    if shape == "narrow":
        k32 = ((code % 61) * 1_000_000 - 5).astype(np.int32)
        k16 = (code // 61 - 20).astype(np.int16)
        v32 = ((code * 7) % 23 != 0) & (rng.random(n) > 0.02)
        v16 = (code % 29 != 4) & (rng.random(n) > 0.02)
        if all_null:
            v32[:] = False
            v16[:] = False
        return [(k32, v32, "int32"), (k16, v16, "int16")]
    if shape == "float64":
        return [(_special_float(code, rank, np.arange(n), np.float64), None, "float64")]
    if shape == "float32_bool":
        return [(_special_float(code // 2, rank, np.arange(n), np.float32), None, "float32"), ((code % 2) == 1, None, "bool")]
    raise ValueError(shape)


def _groupby_values(code, rank, rng):
    """Value columns of one rank, by type name: ~10% NULL at random, every value NULL for the codes with code % 23 == 7 (on every
    rank); floats: NaN for code % 11 == 5 on even ranks only, NaN everywhere for code % 13 == 6 (all-NaN groups)."""
    n = len(code)
    valid = (rng.random(n) > 0.1) & (code % 23 != 7)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    mag = np.exp2(rng.uniform(-1.0, 1.0, n))  # products of a few dozen stay far from underflow
    out = {
        "int8": rng.integers(-128, 128, n).astype(np.int8),
        "int32": rng.integers(-2**31, 2**31, n).astype(np.int32),
        "uint64": rng.integers(0, 2**64, n, dtype=np.uint64),
        "decimal64": rng.integers(-10**12, 10**12, n).astype(np.int64),
        "timestamp_ms": rng.integers(0, 2**41, n).astype(np.int64),
    }
    for name, dt in (("float32", np.float32), ("float64", np.float64)):
        f = (sign * mag).astype(dt)
        f[(code % 11 == 5) & (rank % 2 == 0)] = np.nan
        f[code % 13 == 6] = np.nan
        out[name] = f
    return {k: (v, valid.copy()) for k, v in out.items()}


# (value name, kinds) per request; each inner list is one call. Every kind of one value type is split over two calls: combine_groupby
# merges one partial column per request slot, and the hash groupby takes at most 7 distinct value columns, a float key column
# counting as one (so all eight kinds of one column - 7 partials - over a float key are beyond the merge).
SUMS = ["sum", "product", "sum_of_squares", "mean"]
EXTREMES = ["min", "max", "count_valid", "count_all", "mean"]
GROUPBY_CALLS = [[(vt, kinds)] for vt in ("int8", "int32", "uint64", "float32", "float64") for kinds in (SUMS, EXTREMES)] + [
    # the same column object twice (shuffle_groupby sends it once; combine_groupby's MEAN shares the SUM partial) and a repeated kind
    [("float64", ["sum", "mean", "sum", "max"]), ("float64", ["mean", "min", "count_valid"])],
    [("decimal64", ["sum", "min", "max"]), ("timestamp_ms", ["min", "max"])],
]


def _bounds(kind, vt, m, amax, expected):
    """Per-group absolute bound of a float aggregation (None: exact)."""
    if vt not in ("float32", "float64"):
        return 0.0
    eps = float(np.finfo(np.float32 if vt == "float32" else np.float64).eps)
    m = m.astype(np.float64)
    if kind == "sum":
        return m * m * eps * amax  # == kat.sum_atol(m_g, max|v_g|) in the value type's epsilon
    if kind == "sum_of_squares":
        return m * m * eps * amax * amax
    if kind == "mean":
        return (m + 1) * eps * amax
    if kind == "product":
        with np.errstate(invalid="ignore"):
            return np.nan_to_num(2 * (m + 1) * eps * np.abs(expected[0].astype(np.float64)), nan=0.0, posinf=0.0)
    return None  # min / max / counts: exact


def _groupby_case(oracle, world, shape, include, rows, seed, all_null_keys=False):
    """Both groupby collectives over the same shards, every call of GROUPBY_CALLS, checked against the oracle; returns the number
    of groups of the first call."""
    import kat
    import cudf_amd
    import gpu_backend as G
    from cudf_amd import distributed as D, groupby as gb
    from cudf_amd.types import NullPolicy
    from oracle.oracle import HostColumn
    rng = np.random.default_rng(seed)
    ngroups = 1500
    hkeys, hvals = [], []
    for r in range(world):
        n = rows[r]
        code = rng.integers(0, ngroups, n)
        special = rng.random(n) < 0.03
        code[special] = rng.integers(0, 8, int(special.sum()))  # the special float classes on every rank
        solo = rng.random(n) < 0.01
        code[solo] = ngroups + 50 * r + rng.integers(0, 50, int(solo.sum()))  # groups present on this rank only
        hkeys.append(_groupby_keys(shape, code, r, rng, all_null_keys))
        hvals.append(_groupby_values(code, r, rng))
    dkeys = [cudf_amd.Table([_device(d, v, t) for d, v, t in ks]) for ks in hkeys]
    scale_of = {"decimal64": -2}
    dvals = [{name: _device(d, v, name, scale=scale_of.get(name, 0)) for name, (d, v) in vs.items()} for vs in hvals]
    policy = NullPolicy.INCLUDE if include else NullPolicy.EXCLUDE

    def rank_fn(r, comm, stream):
        out = []
        for call in GROUPBY_CALLS:
            reqs = [gb.GroupByRequest(dvals[r][name], [G.make_aggregation(k) for k in kinds]) for name, kinds in call]
            per_api = {}
            for api in (D.shuffle_groupby, D.combine_groupby):
                uk, res = api(comm, dkeys[r], reqs, null_handling=policy, stream=stream)
                per_api[api.__name__] = ([_fetch(c)[0] for c in uk.columns()], [[_fetch(c) for c in t.columns()] for t in res])
            out.append(per_api)
        return out

    res = run_ranks(world, rank_fn)
    all_keys = [HostColumn(np.concatenate([hk[c][0] for hk in hkeys]),
                           None if hkeys[0][c][1] is None else np.concatenate([hk[c][1] for hk in hkeys]), hkeys[0][c][2])
                for c in range(len(hkeys[0]))]
    n_first = None
    for ci, call in enumerate(GROUPBY_CALLS):
        all_vals = {name: (np.concatenate([hv[name][0] for hv in hvals]), np.concatenate([hv[name][1] for hv in hvals]))
                    for name, _ in call}
        oreq = [(HostColumn(*all_vals[name], name), kinds) for name, kinds in call]
        # per-group inputs of the bounds: rows and the largest finite |v| (a NaN never wins a MAX)
        oreq += [(HostColumn(np.abs(all_vals[name][0]).astype(np.float64), all_vals[name][1], "float64"), ["max", "count_all"])
                 for name, _ in call]
        ekeys, eres = oracle.groupby(all_keys, oreq, include_null_keys=include)
        aligned = {}
        for api in ("shuffle_groupby", "combine_groupby"):
            for r in range(world):
                _check_owned(oracle, world, r, res[r][ci][api][0])
            gkeys = [_cat([res[r][ci][api][0][c] for r in range(world)]) for c in range(len(ekeys))]
            assert [k[2] for k in gkeys] == [k[2] for k in ekeys], f"{api}: key types"
            order = _align(gkeys, ekeys)
            if n_first is None:
                n_first = len(order)
            aligned[api] = []
            for q, (name, kinds) in enumerate(call):
                amax_d, amax_v, _ = eres[len(call) + q][0]
                amax = np.where(amax_v if amax_v is not None else True, np.maximum(np.nan_to_num(amax_d, neginf=0.0), 0.0), 0.0)
                m = eres[len(call) + q][1][0]
                cols = []
                for j, kind in enumerate(kinds):
                    got = _take(_cat([res[r][ci][api][1][q][j][0] for r in range(world)]), order)
                    exp = eres[q][j]
                    what = f"{api} {shape} {name} {kind}"
                    bound = _bounds(kind, name, m, amax, exp)
                    kat.compare_columns(got, exp, what, atol=0.0 if bound is None else bound)
                    if bound is None and np.dtype(got[0].dtype).kind == "f":  # MIN / MAX of floats: bit-exact up to the sign of zero
                        ok = exp[1] if exp[1] is not None else np.ones(len(exp[0]), bool)
                        a, e = got[0][ok], exp[0][ok]
                        assert ((a == e) | (np.isnan(a) & np.isnan(e))).all(), f"{what}: not exact"
                    scales = {res[r][ci][api][1][q][j][1] for r in range(world)}
                    assert scales == {-2 if name == "decimal64" and kind in ("sum", "min", "max") else 0}, f"{what}: scale {scales}"
                    cols.append(got)
                aligned[api].append(cols)
        for q, (name, kinds) in enumerate(call):
            if name in INT_VALUE_TYPES:  # integer inputs: the two collectives agree to the bit
                for j, kind in enumerate(kinds):
                    a, b = aligned["shuffle_groupby"][q][j], aligned["combine_groupby"][q][j]
                    va = np.ones(len(a[0]), bool) if a[1] is None else a[1]
                    vb = np.ones(len(b[0]), bool) if b[1] is None else b[1]
                    assert a[2] == b[2] and np.array_equal(va, vb), f"{name} {kind}: validity / type differ between the collectives"
                    assert np.array_equal(a[0][va].view(np.uint8), b[0][vb].view(np.uint8)), f"{name} {kind}: values differ between the collectives"
    return n_first


def _rows(world, empty_rank):
    base = [9_000, 4_000, 12_000, 3_000, 7_000, 11_000, 5_000, 8_000]
    return [0 if r == empty_rank else base[r] for r in range(world)]


@gpu
@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("shape,include", [("int64", False), ("narrow", False), ("narrow", True), ("float64", False),
                                           ("float32_bool", False)])
def test_groupby_key_shapes_with_peers(gpu, oracle, world, shape, include):
    """shuffle_groupby and combine_groupby over every value type and kind they serve, for each key shape (int64; nullable int32 +
    int16 under EXCLUDE and INCLUDE; float64 with -0.0 on even ranks, +0.0 on odd ones, NaNs of different payloads and signs and
    +-inf; float32 + bool), one rank empty (world > 2), groups on one rank only, all-NULL groups, NaN values on some ranks and
    all-NaN groups (MIN / MAX stay +inf / -inf: test_all_nan_group_min_max_argmin_argmax_pinned)."""
    seed = 1000 + 10 * world + ["int64", "narrow", "float64", "float32_bool"].index(shape) * 100 + include
    _groupby_case(oracle, world, shape, include, _rows(world, world - 1 if world > 2 else None), seed)


@gpu
def test_groupby_all_rows_on_one_rank(gpu, oracle):
    """Every row on rank 2 of 4: its peers send nothing and still receive the groups they own."""
    _groupby_case(oracle, 4, "narrow", True, [0, 0, 30_000, 0], 1901)


@gpu
@pytest.mark.parametrize("include", [False, True])
def test_groupby_all_keys_null(gpu, oracle, include):
    """Every key NULL: EXCLUDE -> no group anywhere; INCLUDE -> one NULL group, on exactly one rank (the owner of the NULL row hash)."""
    n = _groupby_case(oracle, 4, "narrow", include, _rows(4, 3), 1902 + include, all_null_keys=True)
    assert n == (1 if include else 0)


@gpu
@pytest.mark.parametrize("world", [2, 4])
def test_groupby_every_rank_empty(gpu, world):
    """No rows anywhere: zero groups, with the reference's result types (COUNT INT32, MEAN FLOAT64, SUM of an int column INT64)."""
    import cudf_amd
    from cudf_amd import aggregation as agg, distributed as D, groupby as gb
    from cudf_amd.types import NullPolicy, TypeId

    def rank_fn(r, comm, stream):
        keys = cudf_amd.Table([_device(np.zeros(0, np.int32), np.zeros(0, bool), "int32"), _device(np.zeros(0, np.float64), None, "float64")])
        vals = _device(np.zeros(0, np.int32), None, "int32")
        out = []
        for api in (D.shuffle_groupby, D.combine_groupby):
            for policy in (NullPolicy.EXCLUDE, NullPolicy.INCLUDE):
                req = gb.GroupByRequest(vals, [agg.count(NullPolicy.EXCLUDE), agg.count(NullPolicy.INCLUDE), agg.mean(), agg.sum()])
                uk, res = api(comm, keys, [req], null_handling=policy, stream=stream)
                out.append((uk.num_rows(), [c.type().id() for c in uk.columns()], [(c.size(), c.type().id()) for c in res[0].columns()]))
        return out

    for per_rank in run_ranks(world, rank_fn):
        for nrows, ktypes, rtypes in per_rank:
            assert nrows == 0
            assert ktypes == [TypeId.INT32, TypeId.FLOAT64]
            assert rtypes == [(0, TypeId.INT32), (0, TypeId.INT32), (0, TypeId.FLOAT64), (0, TypeId.INT64)]


@gpu
def test_combine_groupby_rejects_every_non_decomposable_kind(gpu):
    """Each kind the header lists as not decomposable (M2, VARIANCE, STD, ARGMIN, ARGMAX, SUM_WITH_OVERFLOW, MEAN of a decimal or a
    duration column) raises ValueError on every rank before the exchange; the same communicator then completes a valid call."""
    import cudf_amd
    from cudf_amd import aggregation as agg, distributed as D, groupby as gb
    world = 4
    keys = [cudf_amd.Table([_device(np.arange(n, dtype=np.int64) % 7, None, "int64")]) for n in (100, 0, 37, 64)]
    f64 = [_device(np.arange(n, dtype=np.float64), None, "float64") for n in (100, 0, 37, 64)]
    dec = [_device(np.arange(n, dtype=np.int64), None, "decimal64", scale=-2) for n in (100, 0, 37, 64)]
    dur = [_device(np.arange(n, dtype=np.int64), None, "duration_ms") for n in (100, 0, 37, 64)]
    bad = [("f64", agg.m2), ("f64", agg.variance), ("f64", agg.std), ("f64", agg.argmin), ("f64", agg.argmax),
           ("f64", agg.sum_with_overflow), ("dec", agg.mean), ("dur", agg.mean)]

    def rank_fn(r, comm, stream):
        cols = {"f64": f64[r], "dec": dec[r], "dur": dur[r]}
        for col, make in bad:
            with pytest.raises(ValueError):
                D.combine_groupby(comm, keys[r], [gb.GroupByRequest(cols[col], [agg.sum(), make()])], stream=stream)
        uk, _ = D.combine_groupby(comm, keys[r], [gb.GroupByRequest(f64[r], [agg.sum(), agg.mean()])], stream=stream)
        return uk.num_rows()

    assert sum(run_ranks(world, rank_fn)) == 7


# ------------------------------------------------------------------ shuffle
def _shuffle_check(oracle, world, res, inputs, key_idx, types):
    """res[r] = [(data, valid, type id), scale, null count] per column; inputs[r] = [(data, valid)] per column (the logical slices)."""
    def rows(cols):
        per_col = []
        for d, v in cols:
            if d.dtype.kind == "f":  # bit patterns: the exchange moves bits, NaN payloads and -0.0 included
                d = d.view(np.uint32 if d.itemsize == 4 else np.uint64)
            vals = d.tolist()
            if v is not None:
                vals = [x if ok else None for x, ok in zip(vals, v.tolist())]
            per_col.append(vals)
        return list(zip(*per_col))

    sent = collections.Counter()
    for cols in inputs:
        sent.update(rows(cols))
    got = collections.Counter()
    for r, cols in enumerate(res):
        assert [c[0][2] for c in cols] == [t for t, _ in types], f"rank {r}: column types"
        assert [c[1] for c in cols] == [s for _, s in types], f"rank {r}: column scales"
        for (d, v, _), _, nulls in cols:
            assert nulls == (0 if v is None else int((~v).sum())), f"rank {r}: null count"
        _check_owned(oracle, world, r, [cols[k][0] for k in key_idx])
        got.update(rows([(d, v) for (d, v, _), _, _ in cols]))
    assert sum(got.values()) == sum(sent.values()), "rows lost or duplicated"
    assert got == sent, "the received rows differ from the sent ones"


@gpu
@pytest.mark.parametrize("world,limit", [(2, None), (4, 16 * 1024), (8, None)])
def test_shuffle_mixed_widths_sliced(gpu, oracle, world, limit):
    """shuffle of bool, int8, int16 (NULLs on rank 0 only), nullable int32, float32 (raw bits: NaN payloads, -0.0), int64,
    decimal64 (scale -2) and timestamp_ms, keyed on (int64, nullable int32); every column of every rank sliced at offset 1, 33 or 67
    (each column its own), one rank empty (world > 2)."""
    import cudf_amd
    from oracle.oracle import TYPE_ID
    rng = np.random.default_rng(3000 + world)
    spec = [("bool", 0), ("int8", 0), ("int16", 0), ("int32", 0), ("float32", 0), ("int64", 0), ("decimal64", -2), ("timestamp_ms", 0)]
    sizes = [40_000, 9_000, 25_000, 3, 17_000, 64, 33, 20_000]
    empty = 1 if world > 2 else None
    inputs, tables = [], []
    for r in range(world):
        n = 0 if r == empty else sizes[r]
        cols, dcols = [], []
        for c, (t, scale) in enumerate(spec):
            off = OFFSETS[(r + c) % 3]
            full = n + off
            data = {"bool": lambda: rng.random(full) < 0.5, "int8": lambda: rng.integers(-128, 128, full).astype(np.int8),
                    "int16": lambda: rng.integers(-2**15, 2**15, full).astype(np.int16),
                    "int32": lambda: rng.integers(-3000, 3000, full).astype(np.int32),
                    "float32": lambda: rng.integers(0, 2**32, full, dtype=np.uint64).astype(np.uint32).view(np.float32),
                    "int64": lambda: rng.integers(-5000, 5000, full).astype(np.int64),
                    "decimal64": lambda: rng.integers(-10**15, 10**15, full).astype(np.int64),
                    "timestamp_ms": lambda: rng.integers(0, 2**42, full).astype(np.int64)}[t]()
            valid = None
            if t == "int32" or (t == "int16" and r == 0):
                valid = rng.random(full) > 0.15
            dcols.append(_device(data, valid, t, offset=off, scale=scale))
            cols.append((data[off:], None if valid is None else valid[off:]))
        inputs.append(cols)
        tables.append(cudf_amd.Table(dcols))
    key_idx = [5, 3]

    def rank_fn(r, comm, stream):
        from cudf_amd import distributed as D
        if limit:
            comm.set_max_message_bytes(limit)
        mine = D.shuffle(comm, tables[r], key_idx, stream=stream)
        return [(*_fetch(c), c.null_count()) for c in mine.columns()]

    res = run_ranks(world, rank_fn)
    assert any(c[0][1] is not None and not c[0][1].all() for r in range(world) for c in res[r][2:3]), "the int16 NULLs travelled"
    _shuffle_check(oracle, world, res, inputs, key_idx, [(TYPE_ID[t], s) for t, s in spec])


def _nullable_table(rng, n, ncols, nullable, off):
    """ncols int32 / float64 / int16 columns sliced at `off`; column c nullable where nullable[c]."""
    kinds = [("int32", np.int32), ("float64", np.float64), ("int16", np.int16)]
    cols, dcols = [], []
    for c in range(ncols):
        t, dt = kinds[c % 3]
        data = (rng.integers(-500, 500, n + off) if dt != np.float64 else rng.integers(-500, 500, n + off) * 0.5).astype(dt)
        valid = (rng.random(n + off) > 0.2) if nullable[c] else None
        dcols.append(_device(data, valid, t, offset=off))
        cols.append((data[off:], None if valid is None else valid[off:]))
    return cols, dcols, [(int(_device(np.zeros(1, dt), None, t).type().id()), 0) for t, dt in (kinds[c % 3] for c in range(ncols))]


@gpu
def test_shuffle_sixteen_flat_columns(gpu, oracle):
    """8 columns, all nullable: 16 flat columns (each validity travels as a byte column), the most the exchange moves - succeeds
    with peers."""
    import cudf_amd
    from cudf_amd import distributed as D
    rng = np.random.default_rng(3100)
    world, sizes = 4, [20_000, 0, 7_000, 13_000]
    inputs, tables, types = [], [], None
    for r in range(world):
        cols, dcols, types = _nullable_table(rng, sizes[r], 8, [True] * 8, OFFSETS[r % 3])
        inputs.append(cols)
        tables.append(cudf_amd.Table(dcols))

    def rank_fn(r, comm, stream):
        mine = D.shuffle(comm, tables[r], [0, 2], stream=stream)
        return [(*_fetch(c), c.null_count()) for c in mine.columns()]

    _shuffle_check(oracle, world, run_ranks(world, rank_fn), inputs, [0, 2], types)


@gpu
def test_shuffle_seventeen_flat_columns_fails_on_every_rank(gpu, monkeypatch):
    """9 columns, 8 of them nullable - the last one only on rank 2, so the other ranks learn of its validity column from the
    round-0 exchange: 17 flat columns. Every rank raises ValueError, none is left waiting (a fresh world: a failed loopback world
    stays failed by design)."""
    import cudf_amd
    from cudf_amd import distributed as D
    monkeypatch.setenv("CUDF_AMD_LOOPBACK_TIMEOUT_S", "10")
    rng = np.random.default_rng(3200)
    world = 4
    tables = []
    for r in range(world):
        nullable = [True] * 7 + [False, r == 2]
        tables.append(cudf_amd.Table(_nullable_table(rng, [500, 0, 70, 300][r], 9, nullable, 1)[1]))

    def rank_fn(r, comm, stream):
        with pytest.raises(ValueError, match="16 flat columns"):
            D.shuffle(comm, tables[r], [0], stream=stream)
        return True

    assert run_ranks(world, rank_fn, timeout=60) == [True] * world


# ------------------------------------------------------------------ shuffle_join
def _join_keys(case, rng, r, n):
    """Key columns [(data, valid, type name)] of one side of one rank."""
    if case == "composite":  # int32 + float64 with -0.0 / +0.0 by rank parity and NaNs of different payloads
        code = rng.integers(0, 12, n)
        return [(rng.integers(0, 1500, n).astype(np.int32), None, "int32"),
                (_special_float(code, r, np.arange(n), np.float64), None, "float64")]
    if case in ("nullable_equal", "nullable_unequal"):
        return [(rng.integers(0, 2000, n).astype(np.int64), rng.random(n) > 0.1, "int64"),
                (rng.integers(0, 4, n).astype(np.int16), rng.random(n) > 0.1, "int16")]
    if case == "duplicated":
        k = rng.integers(0, 5000, n).astype(np.int64)
        k[rng.random(n) < 0.3] = 7
        return [(k, None, "int64")]
    raise ValueError(case)


@gpu
@pytest.mark.parametrize("case,world,limit", [("composite", 2, None), ("composite", 4, None), ("composite", 8, None),
                                              ("nullable_equal", 2, None), ("nullable_unequal", 8, None),
                                              ("duplicated", 4, 16 * 1024)])
def test_shuffle_join_key_shapes_sliced(gpu, oracle, case, world, limit):
    """shuffle_join with composite float keys, nullable keys (NULLs equal and unequal) and one heavily duplicated key, every key
    column sliced at offset 1, 33 or 67: the pairs of oracle.join over the concatenated sides, as global row ids, each once, from the
    rank that owns the key."""
    import kat
    import cudf_amd
    from cudf_amd import distributed as D
    from oracle.oracle import HostColumn
    rng = np.random.default_rng(4000 + 10 * world + ["composite", "nullable_equal", "nullable_unequal", "duplicated"].index(case))
    nulls_equal = case != "nullable_unequal"
    lrows = [9_000, 17, 0, 6_000, 1, 2_500, 700, 4_000]
    rrows = [3_000, 0, 1_200, 5, 2_000, 900, 1, 1_500]
    if case == "duplicated":
        rrows = [r // 8 for r in rrows]
    sides, dsides = [], []
    for rows in (lrows, rrows):
        host, dev = [], []
        for r in range(world):
            cols = _join_keys(case, rng, r, rows[r] + 67)
            off = [OFFSETS[(r + c) % 3] for c in range(len(cols))]
            host.append([(d[o:o + rows[r]], None if v is None else v[o:o + rows[r]], t) for (d, v, t), o in zip(cols, off)])
            dev.append(cudf_amd.Table([_device(d[:o + rows[r]], None if v is None else v[:o + rows[r]], t, offset=o)
                                       for (d, v, t), o in zip(cols, off)]))
        sides.append(host)
        dsides.append(dev)

    def rank_fn(r, comm, stream):
        if limit:
            comm.set_max_message_bytes(limit)
        li, ri = D.shuffle_join(comm, dsides[0][r], dsides[1][r], nulls_equal=nulls_equal, stream=stream)
        return li.to_numpy()[0], ri.to_numpy()[0]

    res = run_ranks(world, rank_fn)
    whole = []
    for host in sides:
        ncols = len(host[0])
        whole.append([HostColumn(np.concatenate([h[c][0] for h in host]),
                                 None if host[0][c][1] is None else np.concatenate([h[c][1] for h in host]), host[0][c][2])
                      for c in range(ncols)])
    from oracle.oracle import TYPE_ID
    for side in (0, 1):
        owner = _owners(oracle, [(h.data, h.valid, h.type_id) for h in whole[side]], world)
        for r, pair in enumerate(res):
            assert (owner[pair[side]] == r).all(), f"rank {r} returned a pair whose key it does not own"
    gl = np.concatenate([a for a, _ in res])
    gr = np.concatenate([b for _, b in res])
    el, er = oracle.join(whole[0], whole[1], nulls_equal=nulls_equal, kind="inner")
    assert len(el) > 0
    assert kat.sorted_pairs(gl, gr) == kat.sorted_pairs(el, er)


# ------------------------------------------------------------------ the checker itself (CPU)
def test_canon_rows_compares_float_keys_as_classes():
    """-0.0 / +0.0 are one class, every NaN (any payload or sign) is one class, NULL rows compare by validity only."""
    from oracle.oracle import TYPE_ID
    nans = np.array([0x7ff8000000000000, 0xfff0000000000123, 0x7ff0000000000001], dtype=np.uint64).view(np.float64)
    d = np.concatenate([[-0.0, 0.0], nans, [np.inf, 1.5, 7.0]])
    v = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    rows = canon_rows([(d, v, TYPE_ID["float64"])])
    assert rows[0] == rows[1] and rows[2] == rows[3] == rows[4]
    assert len(set(rows)) == 5 and rows[7] == (None,)
    assert canon_rows([(np.array([7, 7], np.int16), np.array([0, 1], bool), TYPE_ID["int16"])]) == [(None,), (7,)]
