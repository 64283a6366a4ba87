"""GPU tests of cudf::groupby::groupby::scan and ::replace_nulls through the C ABI (cudf_amd.groupby.GroupBy.scan /
.replace_nulls): the vectors transcribed from the reference's tests, seeded random inputs against the numpy restatement
(tests/scan_restatement.py), size-independent properties at 100M rows, and the rejected inputs.

The contract leaves the order of groups open: groups are contiguous and keep input order inside, so the GPU's groups are matched to
the restatement's by key before anything is compared."""
import zlib

import numpy as np
import pytest

import scan_golden as GD
import scan_restatement as R

pytestmark = pytest.mark.gpu

F32_EPS = float(np.finfo(np.float32).eps)
F64_EPS = float(np.finfo(np.float64).eps)


def _type_ids():
    from cudf_amd.types import TypeId as T
    return {"int8": T.INT8, "int16": T.INT16, "int32": T.INT32, "int64": T.INT64, "uint8": T.UINT8, "uint16": T.UINT16,
            "uint32": T.UINT32, "uint64": T.UINT64, "float32": T.FLOAT32, "float64": T.FLOAT64, "bool": T.BOOL8,
            "decimal32": T.DECIMAL32, "decimal64": T.DECIMAL64, "timestamp_days": T.TIMESTAMP_DAYS,
            "timestamp_ms": T.TIMESTAMP_MILLISECONDS, "duration_days": T.DURATION_DAYS, "duration_s": T.DURATION_SECONDS,
            "duration_ns": T.DURATION_NANOSECONDS}


def to_device(col, pad=0, rng=None):
    """A column on the device; pad > 0 uploads `pad` extra leading rows and slices them off (a column with an offset)."""
    import cudf_amd
    from cudf_amd.types import DataType
    data, valid, t = np.asarray(col[0]), col[1], col[2]
    scale = col[3] if len(col) > 3 else 0
    if pad:
        data = np.concatenate([data[:1].repeat(pad) if len(data) else np.zeros(pad, data.dtype), data])
        if valid is not None:
            valid = np.concatenate([rng.random(pad) < 0.5, valid])
    return cudf_amd.Column.from_numpy(data, valid, dtype=DataType(_type_ids()[t], scale), offset=pad)


def from_device(c):
    data, valid = c.to_numpy()
    return data, valid


def make_agg(spec):
    from cudf_amd import aggregation as A
    from cudf_amd.types import NullOrder, NullPolicy, Order
    spec = {"kind": spec} if isinstance(spec, str) else spec
    k = spec["kind"]
    if k == "rank":
        return A.rank(A.RankMethod[spec.get("method", "first").upper()], Order[spec.get("order", "ascending").upper()],
                      NullPolicy[spec.get("null_handling", "exclude").upper()], NullOrder[spec.get("null_precedence", "after").upper()],
                      A.RankPercentage[spec.get("percentage", "none").upper()])
    return {"sum": A.sum, "product": A.product, "min": A.min, "max": A.max, "mean": A.mean, "nunique": A.nunique,
            "count_valid": lambda: A.count(NullPolicy.EXCLUDE), "count_all": lambda: A.count(NullPolicy.INCLUDE)}[k]()


def groupby_of(keys, include_null_keys, keys_are_sorted, pad=0, rng=None):
    import cudf_amd
    from cudf_amd import groupby as G
    from cudf_amd.types import NullPolicy, Sorted
    kt = cudf_amd.Table([to_device(k, pad, rng) for k in keys])
    return G.GroupBy(kt, NullPolicy.INCLUDE if include_null_keys else NullPolicy.EXCLUDE,
                     Sorted.YES if keys_are_sorted else Sorted.NO)


def gpu_scan(keys, requests, include_null_keys=False, keys_are_sorted=False, pad=0, rng=None):
    from cudf_amd import groupby as G
    g = groupby_of(keys, include_null_keys, keys_are_sorted, pad, rng)
    reqs = [G.GroupByRequest(to_device(v, pad, rng), [make_agg(s) for s in specs]) for v, specs in requests]
    out_keys, results = g.scan(reqs)
    return [from_device(c) for c in out_keys.columns()], [[from_device(c) for c in t.columns()] for t in results]


def gpu_replace_nulls(keys, values, policies, include_null_keys=False, keys_are_sorted=False, pad=0, rng=None):
    import cudf_amd
    from cudf_amd.aggregation import ReplacePolicy
    g = groupby_of(keys, include_null_keys, keys_are_sorted, pad, rng)
    vt = cudf_amd.Table([to_device(v, pad, rng) for v in values])
    out_keys, out = g.replace_nulls(vt, [ReplacePolicy[p.upper()] for p in policies])
    return [from_device(c) for c in out_keys.columns()], [from_device(c) for c in out.columns()]


def _row_ids(cols, types):
    """One bytes object per row identifying its key (nulls equal nulls, NaN == NaN, -0 == +0)."""
    n = len(cols[0][0])
    parts = []
    for (data, valid), t in zip(cols, types):
        v = np.ones(n, bool) if valid is None else np.asarray(valid, bool)
        w = np.where(v, R._words(np.asarray(data), t, True), np.uint64(0))
        parts += [w, v.astype(np.uint64)]
    m = np.ascontiguousarray(np.stack(parts, axis=1)) if n else np.zeros((0, len(parts)), np.uint64)
    return [m[i].tobytes() for i in range(n)]


def group_permutation(got_keys, exp_keys, key_types, keys_are_sorted):
    """Indices that put the GPU's rows in the restatement's order: checks that the GPU's groups are contiguous runs and
    matches them to the restatement's groups by key. Pre-sorted keys keep the rows where they are: the identity."""
    n = len(exp_keys[0][0])
    assert len(got_keys[0][0]) == n, f"{len(got_keys[0][0])} key rows, expected {n}"
    if keys_are_sorted or n == 0:
        return np.arange(n)
    gids, eids = _row_ids(got_keys, key_types), _row_ids([k[:2] for k in exp_keys], key_types)
    runs = {}
    start = 0
    for i in range(1, n + 1):
        if i == n or gids[i] != gids[start]:
            assert gids[start] not in runs, "a group's rows are not contiguous"
            runs[gids[start]] = (start, i)
            start = i
    perm = np.empty(n, dtype=np.int64)
    start = 0
    for i in range(1, n + 1):
        if i == n or eids[i] != eids[start]:
            lo, hi = runs[eids[start]]
            assert hi - lo == i - start, "group sizes differ"
            perm[start:i] = np.arange(lo, hi)
            start = i
    return perm


def _take(col, perm):
    return np.asarray(col[0])[perm], (None if col[1] is None else np.asarray(col[1], bool)[perm])


def check_result(got, exp, spec, what, values=None, order=None, starts=None):
    """Integers, counts, ranks, MIN, MAX: exact (floats bit for bit). Float SUM: within 64 eps of the row's prefix sum of |v|.
    Float PRODUCT: relative, growing with the row's position inside its group."""
    spec = {"kind": spec} if isinstance(spec, str) else spec
    gd, gv = got
    ed, ev = exp[0], exp[1]
    gvalid = np.ones(len(gd), bool) if gv is None else np.asarray(gv, bool)
    evalid = np.ones(len(ed), bool) if ev is None else np.asarray(ev, bool)
    assert np.array_equal(gvalid, evalid), f"{what}: validity differs at {np.flatnonzero(gvalid != evalid)[:8]}"
    gd, ed = np.asarray(gd)[evalid], np.asarray(ed)[evalid]
    rtype = exp[2]
    kind = spec["kind"]
    if R.cls_of(rtype) in ("f32", "f64") and kind in ("sum", "product"):
        eps = F32_EPS if rtype == "float32" else F64_EPS
        e = ed.astype(np.float64)
        g = gd.astype(np.float64)
        if kind == "sum":
            tol = 64 * eps * R.abs_prefix(values, order, starts)[evalid] + np.finfo(np.float64).tiny
        else:
            pos = R.position_in_group(starts)[evalid] + 1
            sub = float(np.finfo(np.float32 if rtype == "float32" else np.float64).smallest_subnormal)
            tol = 4 * pos * (eps * np.abs(e) + sub)  # (products that underflow round in absolute steps)
        with np.errstate(invalid="ignore"):
            bad = ~((np.abs(g - e) <= tol) | (np.isnan(g) & np.isnan(e)) | (g == e))
        assert not bad.any(), f"{what}: {g[bad][:5]} vs {e[bad][:5]} (tol {tol[bad][:5]})"
    elif gd.dtype.kind == "f" and kind == "rank":
        ok = (gd == ed) | np.isclose(gd, ed, rtol=1e-15, atol=0) | (np.isnan(gd) & np.isnan(ed))
        assert ok.all(), f"{what}: {gd[~ok][:8]} vs {ed[~ok][:8]}"
    elif gd.dtype.kind == "f":  # MIN / MAX / replace_nulls: bit for bit
        ok = gd.view(np.uint32 if gd.dtype == np.float32 else np.uint64) == np.asarray(ed, gd.dtype).view(
            np.uint32 if gd.dtype == np.float32 else np.uint64)
        assert ok.all(), f"{what}: {gd[~ok][:8]} vs {ed[~ok][:8]}"
    else:
        ok = gd.astype(np.int64) == np.asarray(ed).astype(np.int64)
        assert ok.all(), f"{what}: {gd[~ok][:8]} vs {np.asarray(ed)[~ok][:8]}"


def compare_scan(keys, requests, include_null_keys=False, keys_are_sorted=False, pad=0, rng=None):
    got_keys, got = gpu_scan(keys, requests, include_null_keys, keys_are_sorted, pad, rng)
    exp_keys, exp = R.scan(keys, requests, include_null_keys, keys_are_sorted)
    order, starts = R.group_order(keys, include_null_keys, keys_are_sorted)
    types = [k[2] for k in keys]
    perm = group_permutation(got_keys, exp_keys, types, keys_are_sorted)
    for i, (gk, ek) in enumerate(zip(got_keys, exp_keys)):
        check_result(_take(gk, perm), ek, "min", f"keys[{i}]")
    for r, (v, specs) in enumerate(requests):
        for j, s in enumerate(specs):
            check_result(_take(got[r][j], perm), exp[r][j], s, f"request {r} ({v[2]}) {s}", v, order, starts)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's vectors

CASES = GD.load_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden(gpu, case):
    keys, values, spec = GD.inputs(case)
    exp_keys, exp = GD.expected(case)
    if spec["kind"] == "replace_nulls":
        got_keys, cols = gpu_replace_nulls(keys, [values], [spec["policy"]], case["include_null_keys"], case["keys_are_sorted"])
        got = cols[0]
    else:
        got_keys, res = gpu_scan(keys, [(values, [spec])], case["include_null_keys"], case["keys_are_sorted"])
        got = res[0][0]
    perm = group_permutation(got_keys, [exp_keys], [case["key_type"]], case["keys_are_sorted"])
    GD.same_column(_take(got_keys[0], perm), exp_keys, "keys")
    GD.same_column(_take(got, perm), exp, "result", exact="percentage" not in spec)


# ---------------------------------------------------------------------------------------------------------------------------------
# seeded random inputs against the restatement

VALUE_TYPES = ["int8", "int16", "int32", "int64", "uint8", "uint32", "uint64", "float32", "float64", "bool", "decimal32",
               "decimal64", "timestamp_ms", "duration_s", "duration_days"]


def random_values(rng, t, n, nulls=0.2):
    dt, c = R.TYPES[t]
    if c == "f32" or c == "f64":
        d = rng.standard_normal(n) * 100
        special = rng.random(n)
        d[special < 0.02] = 0.0
        d[(special >= 0.02) & (special < 0.04)] = -0.0
        d[(special >= 0.04) & (special < 0.05)] = np.nan
        d[(special >= 0.05) & (special < 0.055)] = np.inf
        d = d.astype(dt)
    elif c == "bool":
        d = rng.random(n) < 0.5
    else:
        info = np.iinfo(dt)
        d = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        small = rng.random(n) < 0.5  # ties for MIN / MAX / RANK next to full-range values that wrap SUM / PRODUCT
        d[small] = (d[small] % 7).astype(dt)
    valid = rng.random(n) >= nulls if nulls else None
    return (d, valid, t, -2 if t.startswith("decimal") else 0)


def scan_specs(t):
    """Every scan kind the type supports (float PRODUCT apart: it gets values near 1), and the first of them again."""
    s = [k for k in ("sum", "product", "min", "max", "count_valid", "count_all")
         if R.scan_type(t, k) is not None and not (k == "product" and R.cls_of(t) in ("f32", "f64"))]
    return s + s[:1]


def near_one(rng, t, n):
    d = (rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)).astype(R.TYPES[t][0])
    return (d, rng.random(n) >= 0.2, t)


def key_shape(rng, shape, n):
    if shape == "int32":
        return [(rng.integers(0, 300, n).astype(np.int32), None, "int32")], False, False
    if shape == "sparse_int64":
        return [(rng.choice(rng.integers(-2 ** 62, 2 ** 62, 500, dtype=np.int64), n), None, "int64")], False, False
    if shape == "float64":
        pool = np.array([0.0, -0.0, np.nan, -np.nan, 1.5, -2.25, np.inf, 1e300])
        return [(rng.choice(pool, n), None, "float64")], False, False
    if shape == "two_keys":
        return [(rng.integers(0, 20, n).astype(np.int16), None, "int16"),
                (rng.integers(0, 30, n).astype(np.uint32), None, "uint32")], False, False
    if shape in ("nullable_exclude", "nullable_include"):
        return [(rng.integers(0, 200, n).astype(np.int64), rng.random(n) >= 0.1, "int64"),
                (rng.integers(0, 3, n).astype(np.int8), rng.random(n) >= 0.1, "int8")], shape == "nullable_include", False
    if shape == "presorted":
        return [(np.sort(rng.integers(0, 400, n)).astype(np.int32), None, "int32")], False, True
    if shape == "singletons":
        return [(rng.permutation(n).astype(np.int64), None, "int64")], False, False
    raise AssertionError(shape)


@pytest.mark.parametrize("shape", ["int32", "sparse_int64", "float64", "two_keys", "nullable_exclude", "nullable_include",
                                   "presorted", "singletons"])
def test_random_scans(gpu, shape):
    rng = np.random.default_rng(zlib.crc32(shape.encode()))
    n = 30_000
    keys, include, presorted = key_shape(rng, shape, n)
    requests = [(random_values(rng, t, n, nulls=0.0 if i % 4 == 0 else 0.2), scan_specs(t)) for i, t in enumerate(VALUE_TYPES)]
    requests += [(near_one(rng, "float32", n), ["product"]), (near_one(rng, "float64", n), ["product", "sum"])]
    compare_scan(keys, requests, include, presorted, pad=0 if shape in ("int32", "float64") else 37, rng=rng)


RANK_SPECS = [{"kind": "rank", "method": m, "percentage": p, "order": o, "null_precedence": npr, "null_handling": nh}
              for m in ("first", "average", "min", "max", "dense") for p in ("none", "zero_normalized", "one_normalized")
              for o in ("ascending", "descending") for npr in ("after", "before") for nh in ("exclude", "include")]


@pytest.mark.parametrize("vtype", ["int32", "float64", "bool", "uint16"])
def test_rank_every_option(gpu, vtype):
    rng = np.random.default_rng(7)
    n = 6000
    keys = [(rng.integers(0, 40, n).astype(np.int32), rng.random(n) >= 0.05, "int32")]
    v = random_values(rng, vtype, n, nulls=0.15)
    if vtype != "float64" and vtype != "bool":
        v = ((v[0] % 9).astype(v[0].dtype),) + v[1:]
    for include in (False, True):
        compare_scan(keys, [(v, RANK_SPECS[:60]), (v, RANK_SPECS[60:])], include, False, pad=5, rng=rng)


def test_rank_presorted(gpu):
    rng = np.random.default_rng(11)
    n = 5000
    keys = [(np.sort(rng.integers(0, 60, n)).astype(np.int64), None, "int64")]
    v = (rng.integers(0, 5, n).astype(np.int32), rng.random(n) >= 0.1, "int32")
    compare_scan(keys, [(v, RANK_SPECS)], False, True)


@pytest.mark.parametrize("shape", ["int32", "nullable_exclude", "nullable_include", "presorted"])
def test_replace_nulls_random(gpu, shape):
    rng = np.random.default_rng(3)
    n = 20_000
    keys, include, presorted = key_shape(rng, shape, n)
    types = ["int32", "float64", "int8", "decimal64", "bool", "uint64"]
    values = [random_values(rng, t, n, nulls=0.6) for t in types] + [random_values(rng, "int16", n, nulls=0.0)]
    policies = ["preceding", "following", "following", "preceding", "preceding", "following", "preceding"]
    got_keys, got = gpu_replace_nulls(keys, values, policies, include, presorted, pad=3, rng=rng)
    exp_keys, exp = R.replace_nulls(keys, values, policies, include, presorted)
    perm = group_permutation(got_keys, exp_keys, [k[2] for k in keys], presorted)
    for i, (g, e) in enumerate(zip(got, exp)):
        if values[i][1] is None:
            assert g[1] is None or np.asarray(g[1]).all()
            e = (e[0], None, e[2])
        check_result(_take(g, perm), e, "min", f"column {i} ({types[i] if i < len(types) else 'int16'}, {policies[i]})")


def test_one_group_over_many_tiles(gpu):
    rng = np.random.default_rng(5)
    n = 12_000_000
    k = np.zeros(n, np.int32)
    k[rng.integers(0, n, 1000)] = rng.integers(1, 5, 1000)  # a few rows of other groups inside the big one
    keys = [(k, None, "int32")]
    fv = (rng.random(n), rng.random(n) >= 0.01, "float64")
    iv = (rng.integers(-2 ** 40, 2 ** 40, n), None, "int64")
    compare_scan(keys, [(fv, ["sum", "min", "count_valid"]), (iv, ["sum", "max", "count_all"])])


def test_several_requests_and_repeats(gpu):
    rng = np.random.default_rng(9)
    n = 50_000
    keys = [(rng.integers(0, 1000, n).astype(np.int64), None, "int64")]
    v1 = random_values(rng, "int32", n)
    v2 = random_values(rng, "float32", n)
    specs = ["sum", "sum", "min", "max", "count_all", "count_valid", "product", "max", "sum", "min", "count_all"]  # > 8 kinds
    compare_scan(keys, [(v1, specs), (v2, ["sum", "sum"]), (v1, ["min", {"kind": "rank", "method": "dense"}, "sum"])])


# ---------------------------------------------------------------------------------------------------------------------------------
# properties at 100M rows (the restatement would take too long), checked on the device


def test_properties_100m(gpu):
    import torch
    import cudf_amd
    from cudf_amd import groupby as G
    from cudf_amd.types import DataType, TypeId

    n, groups = 100_000_000, 1_000_000
    gen = torch.Generator(device="cuda").manual_seed(1)
    k = torch.randint(0, groups, (n,), device="cuda", dtype=torch.int64, generator=gen) * 7919
    v = torch.randint(-1000, 1000, (n,), device="cuda", dtype=torch.int32, generator=gen)
    ones = torch.ones(n, device="cuda", dtype=torch.int8)
    kt = cudf_amd.Table([cudf_amd.Column.from_torch(k, dtype=DataType(TypeId.INT64))])
    vc = cudf_amd.Column.from_torch(v, dtype=DataType(TypeId.INT32))
    oc = cudf_amd.Column.from_torch(ones, dtype=DataType(TypeId.INT8))
    g = G.GroupBy(kt)
    from cudf_amd import aggregation as A
    sk, res = g.scan([G.GroupByRequest(vc, [A.count(), A.sum()]), G.GroupByRequest(oc, [A.sum()])])
    keys = sk.columns()[0].to_torch()
    count_all, sums = res[0].columns()[0].to_torch(), res[0].columns()[1].to_torch()
    ones_sum = res[1].columns()[0].to_torch()
    assert keys.numel() == n
    starts = torch.ones(n, dtype=torch.bool, device="cuda")
    starts[1:] = keys[1:] != keys[:-1]
    idx = torch.arange(n, device="cuda")
    first = torch.cummax(torch.where(starts, idx, torch.zeros_like(idx)), 0).values
    assert torch.equal(count_all.to(torch.int64), idx - first + 1), "COUNT_ALL is not 1..size in every group"
    assert torch.equal(ones_sum, count_all.to(torch.int64)), "a SUM scan of ones differs from COUNT_ALL"
    n_groups = int(starts.sum())
    assert n_groups == torch.unique(k).numel(), "a group's rows are not contiguous"
    last = torch.ones(n, dtype=torch.bool, device="cuda")
    last[:-1] = starts[1:]
    uk, ar = g.aggregate([G.GroupByRequest(vc, [A.sum()])])
    ak, asum = uk.columns()[0].to_torch(), ar[0].columns()[0].to_torch()
    order = torch.argsort(ak)
    pos = torch.searchsorted(ak[order], keys[last])
    assert torch.equal(asum[order][pos], sums[last]), "the last SUM scan row of a group differs from the aggregate SUM"


# ---------------------------------------------------------------------------------------------------------------------------------
# the aggregate path after a scan, and the rejected inputs


def test_aggregate_unchanged_after_scan(gpu):
    from cudf_amd import aggregation as A
    from cudf_amd import groupby as G
    rng = np.random.default_rng(2)
    n = 100_000
    keys = [(rng.integers(0, 5000, n).astype(np.int64), None, "int64")]
    v = to_device((rng.integers(-10 ** 9, 10 ** 9, n), None, "int64"))  # integer SUM: the same bits whatever the atomics' order
    g = groupby_of(keys, False, False)

    def agg():
        uk, res = g.aggregate([G.GroupByRequest(v, [A.sum(), A.max()])])
        k = uk.columns()[0].to_numpy()[0]
        o = np.argsort(k)
        return k[o], [c.to_numpy()[0][o] for c in res[0].columns()], g.last_path

    before = agg()
    g.scan([G.GroupByRequest(v, [A.sum(), A.rank(A.RankMethod.DENSE)])])
    after = agg()
    assert after[2] == before[2]
    assert np.array_equal(after[0], before[0])
    for a, b in zip(after[1], before[1]):
        assert np.array_equal(a, b)


def test_empty_and_all_null_keys(gpu):
    empty = [(np.zeros(0, np.int32), None, "int32")]
    specs = ["sum", "count_all", {"kind": "rank", "method": "average"}, "min"]
    k, res = gpu_scan(empty, [((np.zeros(0, np.int16), None, "int16"), specs)])
    assert len(k[0][0]) == 0 and [len(r[0]) for r in res[0]] == [0, 0, 0, 0]
    null_keys = [(np.arange(5, dtype=np.int32), np.zeros(5, bool), "int32")]
    k, res = gpu_scan(null_keys, [((np.arange(5, dtype=np.int64), None, "int64"), specs)])
    assert len(k[0][0]) == 0 and [len(r[0]) for r in res[0]] == [0, 0, 0, 0]
    k, cols = gpu_replace_nulls(null_keys, [(np.arange(5, dtype=np.int64), np.ones(5, bool), "int64")], ["preceding"])
    assert len(k[0][0]) == 0 and len(cols[0][0]) == 0


@pytest.mark.parametrize("bad", [("int32", "mean"), ("int32", "nunique"), ("timestamp_ms", "sum"), ("decimal64", "product"),
                                 ("timestamp_days", "product")])
def test_rejected_kind_or_type(gpu, bad):
    import cudf_amd
    t, kind = bad
    keys = [(np.array([1, 1, 2], np.int32), None, "int32")]
    with pytest.raises(cudf_amd._lib.CudfAmdError):
        gpu_scan(keys, [((np.array([1, 2, 3], R.TYPES[t][0]), None, t), [kind])])


def test_mismatched_sizes(gpu):
    import cudf_amd
    keys = [(np.array([1, 1, 2], np.int32), None, "int32")]
    with pytest.raises(cudf_amd._lib.CudfAmdError):
        gpu_scan(keys, [((np.array([1, 2], np.int64), None, "int64"), ["sum"])])
    with pytest.raises(cudf_amd._lib.CudfAmdError):
        gpu_replace_nulls(keys, [(np.array([1, 2], np.int64), np.array([1, 0], bool), "int64")], ["preceding"])
    with pytest.raises(cudf_amd._lib.CudfAmdError):  # one policy per column
        gpu_replace_nulls(keys, [(np.array([1, 2, 3], np.int64), np.array([1, 0, 1], bool), "int64")] * 2, ["preceding"])
