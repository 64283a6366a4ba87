"""Plain numpy restatement of cudf::groupby::groupby::scan and ::replace_nulls (reference cpp/src/groupby/sort/scan.cpp,
group_scan_util.cuh, group_rank_scan.cu, group_replace_nulls.cu, sort_helper.cu), the checker of tests/test_groupby_scan_gpu.py.

A column is a tuple (data, valid, type_name[, scale]): `valid` is a bool array or None (no null mask). Results come back in one
group order - groups by ascending key (nulls last), input order inside a group - or, for pre-sorted keys, in input order. The
contract leaves the order of groups open; the GPU test matches groups by key before it compares.

Rules restated here:
  * rows: under null_policy EXCLUDE a row with a null in any key column is dropped; with sorted::YES (and nothing to drop) the rows
    stay where they are and the groups are the runs of equal adjacent keys; otherwise the groups are the distinct keys.
  * SUM / PRODUCT / MIN / MAX: inclusive scan inside each group, a null counting as the kind's identity; the result carries the
    grouped values' null mask. Integer SUM / PRODUCT wrap as two's complement (INT64 for plain integers and bools; decimals and
    durations keep their type and wrap in it). MIN / MAX order floats by sign and magnitude: -0 before +0, every NaN above +inf
    and equal to every other NaN; a NaN result is the canonical quiet NaN.
  * COUNT_VALID / COUNT_ALL: INT32 running counts, no mask.
  * RANK: over the group's rows in (value, null) order by column_order (a DESCENDING column flips nulls too: nulls come first
    when null_precedence BEFORE differs from DESCENDING); ties keep input order; with sorted::YES the rows are taken as ordered
    already. Equal values (nulls equal nulls; NaN == NaN, -0 == +0) form runs. FIRST = position + 1, MIN / MAX = the run's first
    / last position + 1, AVERAGE = MIN + (MAX - MIN) / 2, DENSE = runs so far. Percentages divide by the group's valid count
    (EXCLUDE on a nullable column) or its size: ZERO_NORMALIZED r / count, ONE_NORMALIZED (r - 1) / (count - 1) (0 for a count of
    1); DENSE divides by the dense rank found at value-order position (group start + count - 1) instead (1 if that is negative).
    EXCLUDE puts the grouped values' null mask on the result. INT32, or FLOAT64 for AVERAGE and every percentage.
  * replace_nulls: a null takes the nearest valid value before (PRECEDING) or after (FOLLOWING) it inside its group, else stays
    null; a column without a null mask comes back gathered, without one.
"""
import numpy as np

# type name -> (numpy dtype of the data, class)
TYPES = {
    "int8": (np.int8, "sint"), "int16": (np.int16, "sint"), "int32": (np.int32, "sint"), "int64": (np.int64, "sint"),
    "uint8": (np.uint8, "uint"), "uint16": (np.uint16, "uint"), "uint32": (np.uint32, "uint"), "uint64": (np.uint64, "uint"),
    "float32": (np.float32, "f32"), "float64": (np.float64, "f64"), "bool": (np.bool_, "bool"),
    "decimal32": (np.int32, "sint"), "decimal64": (np.int64, "sint"),
    "timestamp_days": (np.int32, "sint"), "timestamp_ms": (np.int64, "sint"),
    "duration_days": (np.int32, "sint"), "duration_s": (np.int64, "sint"), "duration_ns": (np.int64, "sint"),
}
PLAIN = {"int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "bool"}
_TOP = np.uint64(1 << 63)


def cls_of(t):
    return TYPES[t][1]


def scan_type(t, kind, rank=None):
    """Result type of a scan kind over type t, or None where the pair is not supported."""
    c = cls_of(t)
    if kind in ("count_valid", "count_all"):
        return "int32"
    if kind == "rank":
        return "float64" if rank.get("method") == "average" or rank.get("percentage", "none") != "none" else "int32"
    if kind in ("min", "max"):
        return t
    if kind == "sum":
        if c in ("f32", "f64") or t.startswith("decimal") or t.startswith("duration"):
            return t
        return "int64" if t in PLAIN else None
    if kind == "product":
        if c in ("f32", "f64"):
            return t
        return "int64" if t in PLAIN else None
    return None


def _words(data, t, zero_equal):
    """Order-preserving uint64 words; NaN canonical and above +inf; zero_equal: -0 and +0 one word."""
    c = cls_of(t)
    if c == "sint":
        return data.astype(np.int64).view(np.uint64) ^ _TOP
    if c in ("uint", "bool"):
        return data.astype(np.uint64)
    if c == "f32":
        d = data.astype(np.float32).copy()
        if zero_equal:
            d[d == 0] = 0.0
        d[np.isnan(d)] = np.float32("nan")
        b = d.view(np.uint32).astype(np.uint64)
        return np.where(b >> np.uint64(31), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))
    d = data.astype(np.float64).copy()
    if zero_equal:
        d[d == 0] = 0.0
    d[np.isnan(d)] = np.float64("nan")
    b = d.view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b | _TOP)


def _unword(w, t):
    c = cls_of(t)
    dt = TYPES[t][0]
    if c == "sint":
        return (w ^ _TOP).view(np.int64).astype(dt)
    if c in ("uint", "bool"):
        return w.astype(dt)
    if c == "f32":
        b = np.where(w >> np.uint64(31), w ^ np.uint64(0x80000000), ~w & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        return b.view(np.float32)
    return np.where(w >> np.uint64(63), w ^ _TOP, ~w).view(np.float64)


def seg_scan(x, starts, op):
    """Inclusive scan of x by segments (a segment begins where starts is True) with an associative ufunc."""
    x = np.array(x, copy=True)
    seg = np.cumsum(starts)
    d = 1
    with np.errstate(over="ignore", invalid="ignore"):
        while d < len(x):
            same = seg[d:] == seg[:-d]
            x[d:] = np.where(same, op(x[:-d], x[d:]), x[d:])
            d *= 2
    return x


def _valid(col):
    return np.ones(len(col[0]), dtype=bool) if col[1] is None else np.asarray(col[1], dtype=bool)


def group_order(keys, include_null_keys=False, keys_are_sorted=False):
    """(order, starts): the rows in group order and where each group starts."""
    n = len(keys[0][0])
    any_null = np.zeros(n, dtype=bool)
    for k in keys:
        any_null |= ~_valid(k)
    rows = np.arange(n)
    drop = not include_null_keys and any_null.any()
    words = [np.where(_valid(k), _words(np.asarray(k[0]), k[2], True), np.uint64(0)) for k in keys]
    nulls = [~_valid(k) for k in keys]
    if keys_are_sorted and not drop:
        order = rows
    else:
        if drop:
            rows = rows[~any_null]
        sort_keys = [np.arange(len(rows))]
        for w, nl in zip(reversed(words), reversed(nulls)):
            sort_keys += [w[rows], nl[rows]]
        order = rows[np.lexsort(sort_keys)]
    starts = np.zeros(len(order), dtype=bool)
    if len(order):
        starts[0] = True
        for w, nl in zip(words, nulls):
            a, b = order[1:], order[:-1]
            starts[1:] |= (nl[a] != nl[b]) | (~nl[a] & (w[a] != w[b]))
    return order, starts


def _gather(col, order):
    data = np.asarray(col[0])[order]
    valid = None if col[1] is None else np.asarray(col[1], dtype=bool)[order]
    return (data, valid) + tuple(col[2:])


def _rank(gv, gvalid, nullable, starts, spec, presorted):
    n = len(gv[0])
    t = gv[2]
    method = spec.get("method", "first")
    desc = spec.get("order", "ascending") == "descending"
    nulls_first = (spec.get("null_precedence", "after") == "before") != desc
    include = spec.get("null_handling", "exclude") == "include"
    pct = spec.get("percentage", "none")
    seg = np.cumsum(starts) - 1
    gstart = np.flatnonzero(starts)
    gend = np.r_[gstart[1:], n]
    w = np.where(gvalid, _words(np.asarray(gv[0]), t, True), np.uint64(0))
    if desc:
        w = ~w
    nflag = (gvalid if nulls_first else ~gvalid).astype(np.int64)
    vorder = np.arange(n) if presorted else np.lexsort([np.arange(n), w, nflag, seg])
    vw, vvalid = w[vorder], gvalid[vorder]
    pos = np.arange(n)
    gs = gstart[seg]
    run_start = np.ones(n, dtype=bool)
    run_start[1:] = (seg[1:] != seg[:-1]) | (vvalid[1:] != vvalid[:-1]) | (vvalid[1:] & (vw[1:] != vw[:-1]))
    first_of_run = np.maximum.accumulate(np.where(run_start, pos, 0))
    run_id = np.cumsum(run_start) - 1
    run_last = np.r_[np.flatnonzero(run_start)[1:], n][run_id] - 1
    rmin = first_of_run - gs + 1
    rmax = run_last - gs + 1
    dense = run_id - run_id[gs] + 1
    r = {"first": pos - gs + 1, "min": rmin, "max": rmax, "dense": dense,
         "average": rmin + (rmax - rmin) / 2.0}[method]
    if pct != "none":
        if nullable and not include:
            count = np.add.reduceat(vvalid.astype(np.int64), gstart)[seg] if n else np.zeros(0, np.int64)
        else:
            count = (gend - gstart)[seg]
        r = np.asarray(r, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            if method == "dense":
                idx = gs + count - 1
                last = np.where(idx < 0, 1, dense[np.clip(idx, 0, max(n - 1, 0))]).astype(np.float64)
                r = r / last if pct == "zero_normalized" else np.where(last == 1, 0.0, (r - 1.0) / (last - 1))
            else:
                r = r / count if pct == "zero_normalized" else np.where(count == 1, 0.0, (r - 1.0) / (count - 1))
    out = np.empty(n, dtype=np.float64 if (method == "average" or pct != "none") else np.int32)
    out[vorder] = r
    return out, (None if include or not nullable else gvalid.copy())


def scan_one(values, order, starts, spec, presorted=False):
    """One scan aggregation over `values` (a column), given the group order. spec: a kind name or {"kind": ...}."""
    spec = {"kind": spec} if isinstance(spec, str) else spec
    kind = spec["kind"]
    t = values[2]
    gv = _gather(values, order)
    gvalid = _valid(gv)
    nullable = values[1] is not None
    rtype = scan_type(t, kind, spec)
    assert rtype is not None, (t, kind)
    if kind == "count_all":
        return seg_scan(np.ones(len(order), np.int64), starts, np.add).astype(np.int32), None, rtype
    if kind == "count_valid":
        return seg_scan(gvalid.astype(np.int64), starts, np.add).astype(np.int32), None, rtype
    if kind == "rank":
        data, valid = _rank(gv, gvalid, nullable, starts, spec, presorted)
        return data, valid, rtype
    mask = gvalid.copy() if nullable else None
    c = cls_of(t)
    d = np.asarray(gv[0])
    if kind in ("min", "max"):
        w = _words(d, t, False)
        w = np.where(gvalid, w, np.uint64(~np.uint64(0)) if kind == "min" else np.uint64(0))
        w = seg_scan(w, starts, np.minimum if kind == "min" else np.maximum)
        return _unword(w, t), mask, rtype
    if c in ("f32", "f64"):  # float SUM / PRODUCT, restated in float64
        x = np.where(gvalid, d.astype(np.float64), 0.0 if kind == "sum" else 1.0)
        with np.errstate(over="ignore"):
            out = seg_scan(x, starts, np.add if kind == "sum" else np.multiply).astype(TYPES[rtype][0])
        return out, mask, rtype
    x = np.where(gvalid, d.astype(np.int64), 0 if kind == "sum" else 1).astype(np.int64)
    out = seg_scan(x, starts, np.add if kind == "sum" else np.multiply)
    return out.astype(TYPES[rtype][0]), mask, rtype


def abs_prefix(values, order, starts):
    """Per group-order row: the sum of |v| over its group's prefix (the scale of a float SUM's rounding)."""
    gv = _gather(values, order)
    x = np.where(_valid(gv), np.abs(np.asarray(gv[0]).astype(np.float64)), 0.0)
    return seg_scan(x, starts, np.add)


def position_in_group(starts):
    """0-based position of every group-order row inside its group."""
    n = len(starts)
    return np.arange(n) - np.maximum.accumulate(np.where(starts, np.arange(n), 0))


def scan(keys, requests, include_null_keys=False, keys_are_sorted=False):
    """keys: list of columns; requests: list of (values column, [specs]). Returns (keys in group order, [[result]...])."""
    order, starts = group_order(keys, include_null_keys, keys_are_sorted)
    presorted = bool(keys_are_sorted)
    out_keys = [_gather(k, order) for k in keys]
    return out_keys, [[scan_one(v, order, starts, s, presorted) for s in specs] for v, specs in requests]


def replace_nulls(keys, values, policies, include_null_keys=False, keys_are_sorted=False):
    """values: list of columns; policies: "preceding" / "following" per column."""
    order, starts = group_order(keys, include_null_keys, keys_are_sorted)
    out = []
    n = len(order)
    for col, policy in zip(values, policies):
        gv = _gather(col, order)
        if col[1] is None:
            out.append(gv)
            continue
        valid = _valid(gv)
        idx = np.arange(n)
        if policy == "preceding":
            src = seg_scan(np.where(valid, idx, -1), starts, np.maximum)
        else:
            ends = np.r_[starts[1:], True] if n else starts
            src = seg_scan(np.where(valid, idx, -1)[::-1].copy(), ends[::-1].copy(),
                           lambda a, b: np.where(b >= 0, b, a))[::-1]
        ok = src >= 0
        data = np.asarray(gv[0])[np.where(ok, src, 0)] if n else np.asarray(gv[0])
        out.append((data, ok) + tuple(col[2:]))
    return [_gather(k, order) for k in keys], out
