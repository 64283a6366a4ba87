"""Every route of the sort-based groupby (radix_sort.hip, sort_helper.hip, sort_aggregate.hip), each forced by its inputs, compared
with the vectorised numpy reference (tests/sort_reference.py, held to the pinned restatement by tests/test_sort_reference.py) and
ASSERTED from the launch counts of profile_report(): `sort_words` counts the fills of value and label words (one per key column,
one per column sorted ahead of the keys, two per value order sorted afterwards), `sort_scatter` / `sort_hist` the radix passes -
one per byte in which the words of a fill differ.

Integers, order statistics and key BITS are compared exactly (the key of a group is that of its first row in input order, as the
reference's stable sort returns it); interpolated quantiles by kat's 4-ulp rule."""
import numpy as np
import pytest

import kat
import sort_reference as R
from oracle import sort_groupby as SG
from oracle.oracle import HostColumn

pytestmark = pytest.mark.gpu

ORDER_KINDS = ("median", "quantile", "nunique")


@pytest.fixture(scope="module")
def G(gpu):
    import gpu_backend
    return gpu_backend


# ---------------------------------------------------------------- what a call must launch, from its inputs
def radix_words(col):
    """The words the sorter sorts a column by: oracle.sort_groupby.sortable_words, except that a float32 column is ordered in its own
    32 bits (sortable_words widens it to float64, which keeps the order but not the bytes)."""
    words, valid = SG.sortable_words(col)
    data, _ = SG._logical(col)
    if data.dtype == np.float32:
        d = np.where(data == 0, np.float32(0), data)
        bits = d.view(np.uint32).copy()
        bits[np.isnan(d)] = np.uint32(0x7fc00000)
        bits = np.where(bits >> np.uint32(31) != 0, ~bits, bits | np.uint32(1 << 31))
        words = np.where(valid, bits.astype(np.uint64), np.uint64(0))
    return words, valid


def differing_bytes(words):
    """The bytes in which OR and AND of the words differ: the radix passes a sort by these words needs."""
    words = np.asarray(words, np.uint64)
    if len(words) == 0:
        return set()
    d = int(np.bitwise_or.reduce(words) ^ np.bitwise_and.reduce(words))
    return {b for b in range(8) if (d >> (8 * b)) & 0xff}


def _column_passes(col, rows=slice(None)):
    words, valid = radix_words(col)
    passes = len(differing_bytes(words[rows]))
    if col.null_count:  # the null flags are a sort of their own
        passes += len(differing_bytes((~valid[rows]).astype(np.uint64)))
    return passes


_last_groups = [None, None]


def groups_of(keys, include, keys_are_sorted):
    """R.Groups of these very column objects (the last one asked for is kept: a test calls the product several times on the same keys)."""
    tag = (tuple(id(k) for k in keys), include, keys_are_sorted)
    if _last_groups[0] != tag:
        _last_groups[:] = [tag, R.Groups(keys, include, keys_are_sorted), list(keys)]  # (the columns are held, so no id is reused)
    return _last_groups[1]


def expected_launches(keys, requests, include, keys_are_sorted=False):
    """{scope: launches} of one call: sort_helper's plan restated on the inputs."""
    g = groups_of(keys, include, keys_are_sorted)
    keys = [SG._as_host(k) for k in keys]
    specs = [(v, [SG._spec(a) for a in aggs]) for v, aggs in requests]
    any_null = np.zeros(keys[0].size, bool)
    for k in keys:
        any_null |= ~SG._logical(k)[1]
    keys_have_nulls = any(k.null_count for k in keys)
    presorted = keys_are_sorted and not (not include and keys_have_nulls)
    any_nth = any(a["kind"] == "nth_element" for _, aggs in specs for a in aggs)
    order_cols = []  # the columns whose order inside the groups is read, once each
    for v, aggs in specs:
        if any(a["kind"] in ORDER_KINDS for a in aggs) and not any(v is c for c in order_cols):
            order_cols.append(v)
    inner = order_cols[0] if order_cols and not any_nth and not presorted else None
    fills = passes = 0
    if not presorted:
        if inner is not None:  # the one-sort route: this column's words ahead of the keys
            fills += 1
            passes += _column_passes(inner)
        for k in keys:
            fills += 1
            passes += _column_passes(k)
        if not include and keys_have_nulls:
            passes += len(differing_bytes(any_null.astype(np.uint64)))
    if g.num_keys:
        for c in order_cols:
            if c is inner:
                continue
            words, valid = radix_words(c)
            fills += 2
            label_null = (g.labels.astype(np.uint64) << np.uint64(1)) | (~valid[g.order]).astype(np.uint64)
            passes += len(differing_bytes(words[g.order])) + len(differing_bytes(label_null))
    return {"sort_words": fills, "sort_scatter": passes, "sort_hist": passes, "sort_boundaries": 1}


def launches_of(fn):
    from cudf_amd import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
    finally:
        _lib.profile_enable(False)
    return out, {k: v[0] for k, v in _lib.profile_report().items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1) if len(a) else a.reshape(0, 0)


def check_call(G, keys, requests, include=False, keys_are_sorted=False, expect=None):
    """One product call: its launches are those the inputs call for, its results those of the reference. Returns (got, reference)."""
    got, launches = launches_of(lambda: G.groupby(keys, requests, include_null_keys=include, keys_are_sorted=keys_are_sorted))
    assert G.last_path.name == "SORT"
    want = expected_launches(keys, requests, include, keys_are_sorted)
    want.update(expect or {})
    assert {k: launches.get(k, 0) for k in want} == want, launches
    assert launches.get("sort_scan", 0) >= want["sort_scatter"] + 1  # one scan per pass, one for the labels
    exp = R.groupby(keys, requests, include_null_keys=include, keys_are_sorted=keys_are_sorted, groups=groups_of(keys, include, keys_are_sorted))
    gk, gr = got
    assert len(gk) == len(exp.keys)
    for c, (a, e) in enumerate(zip(gk, exp.keys)):
        kat.compare_columns(a, e, f"key column {c}")
        ok = np.ones(len(e[0]), bool) if e[1] is None else e[1]
        assert np.array_equal(_bits(a[0])[ok], _bits(e[0])[ok]), f"key column {c}: not the bits of the group's first row in input order"
    for r, ((_, aggs), ga, ea) in enumerate(zip(requests, gr, exp.results)):
        assert len(ga) == len(ea)
        for j, (spec, a, e) in enumerate(zip(aggs, ga, ea)):
            kat.compare_columns(a, e, f"request {r} aggregation {j} {spec}")
            if SG._spec(spec)["kind"] == "nth_element":  # a pick, not arithmetic: bit for bit
                ok = np.ones(len(e[0]), bool) if e[1] is None else e[1]
                assert np.array_equal(_bits(a[0])[ok], _bits(e[0])[ok]), f"request {r} aggregation {j} {spec}: not bit-equal"
    return got, exp


def identical(a, b, what):
    assert a[2] == b[2] and a[0].tobytes() == b[0].tobytes(), f"{what}: data differ"
    assert (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1])), f"{what}: validity differs"


# ---------------------------------------------------------------- one sort against two
ORDER_READERS_1 = [{"kind": "median"}, {"kind": "nunique"}, {"kind": "quantile", "quantiles": [0.5, 0.37], "interpolation": "midpoint"},
                   {"kind": "nunique", "null_policy": "include"}]
ORDER_READERS_2 = [{"kind": "quantile", "quantiles": [0.0, 0.1, 0.9, 1.0]}, {"kind": "nunique"}, "count_all"]
ORDER_READERS_3 = [{"kind": "quantile", "quantiles": [0.33], "interpolation": "lower"}, {"kind": "quantile", "quantiles": [0.125], "interpolation": "nearest"}]
NTH = [{"kind": "nth_element", "n": 0}, {"kind": "nth_element", "n": -1, "null_policy": "exclude"}]


@pytest.mark.parametrize("n", [20_011, 300_007])
@pytest.mark.parametrize("include", [False, True], ids=["exclude", "include"])
@pytest.mark.parametrize("key_types", [("int32",), ("int64",), ("float64",), ("float32", "int8"), ("uint16", "int64", "bool")], ids="-".join)
def test_one_sort_and_two_sort_routes(G, key_types, include, n):
    """Without an NTH_ELEMENT the first order-reading request's column is sorted ahead of the keys (one fill, no label fill for it);
    the other column still takes a (value, label) sort of its own; a column named twice is sorted once. With an NTH_ELEMENT both
    columns take the second sort. Whatever the route, the same answers."""
    rng = np.random.default_rng(sum(ord(c) for c in "".join(key_types)) + n + (5000 if include else 0))
    keys = [R.random_column(rng, n, t, 9 if len(key_types) > 1 else max(301, n // 60), 0.07) for t in key_types]
    nullable = R.random_column(rng, n, "int64", 50, 0.2)
    plain = R.random_column(rng, n, "float64", 1000, 0.0)
    nk = len(keys)
    one_a = [(nullable, ORDER_READERS_1), (plain, ORDER_READERS_2), (nullable, ORDER_READERS_3)]
    one_b = [(plain, ORDER_READERS_2), (nullable, ORDER_READERS_1 + ORDER_READERS_3)]
    two = [(nullable, ORDER_READERS_1 + NTH), (plain, ORDER_READERS_2), (nullable, ORDER_READERS_3)]
    (_, ra), _ = check_call(G, keys, one_a, include, expect={"sort_words": 1 + nk + 2})
    (_, rb), _ = check_call(G, keys, one_b, include, expect={"sort_words": 1 + nk + 2})
    (_, rt), _ = check_call(G, keys, two, include, expect={"sort_words": nk + 2 + 2})
    for j in range(len(ORDER_READERS_1)):
        identical(ra[0][j], rt[0][j], f"nullable column, aggregation {j}, one sort against two")
        identical(ra[0][j], rb[1][j], f"nullable column, aggregation {j}, sorted ahead of the keys against after them")
    for j in range(len(ORDER_READERS_2)):
        identical(ra[1][j], rt[1][j], f"plain column, aggregation {j}, one sort against two")
        identical(ra[1][j], rb[0][j], f"plain column, aggregation {j}, sorted after the keys against ahead of them")
    for j in range(len(ORDER_READERS_3)):
        identical(ra[2][j], rt[2][j], f"nullable column again, aggregation {j}")


# ---------------------------------------------------------------- the key a group returns
@pytest.mark.parametrize("route", ["one_sort", "two_sort"])
@pytest.mark.parametrize("key_type", ["float64", "float32"])
def test_key_representative_is_the_first_row_of_the_group(G, key_type, route):
    """-0.0 and 0.0 are one key, and so are all NaNs: the key returned is that of the group's first row in input order (the reference
    sorts stably, sort_helper.cu:95-111), bit for bit, on both routes."""
    rng = np.random.default_rng(41 if key_type == "float64" else 42)
    n = 20_011
    ft, ut = (np.float64, np.uint64) if key_type == "float64" else (np.float32, np.uint32)
    nans = np.array([0x7ff8000000000000, 0xfff0000000000abc] if ft == np.float64 else [0x7fc00000, 0xff800abc], ut).view(ft)
    pool = np.concatenate([np.array([-0.0, 0.0], ft), nans, rng.normal(size=12).astype(ft)])
    k = pool[rng.integers(0, len(pool), n)]
    k[:4] = [0.0, nans[1], 1.5, -0.0]  # the zero group opens with +0.0 and the NaN group with the signed payload ...
    second = HostColumn(rng.integers(0, 3, n).astype(np.int8))  # ... and behind a second key column every group has its own opening
    v = HostColumn(rng.normal(size=n))  # the smallest value of a group lies anywhere in it
    aggs = [{"kind": "median"}, {"kind": "nunique"}] + ([{"kind": "nth_element", "n": 0}] if route == "two_sort" else [])
    for keys in ([HostColumn(k)], [HostColumn(k), second], [second, HostColumn(k)]):
        (gk, _), exp = check_call(G, keys, [(v, aggs)], expect={"sort_words": len(keys) + (1 if route == "one_sort" else 2)})
        col = [i for i, c in enumerate(keys) if c is not second][0]
        assert np.array_equal(gk[col][0].view(ut), k[exp.first_rows].view(ut))
        if len(keys) == 1:  # rows 0 and 1 open the zero group and the NaN group
            returned = gk[0][0].view(ut)
            assert np.array([0.0], ft).view(ut)[0] in returned and np.array([-0.0], ft).view(ut)[0] not in returned
            assert nans[1:].view(ut)[0] in returned and nans[:1].view(ut)[0] not in returned


# ---------------------------------------------------------------- which digits are sorted
def _int64_keys_differing_in(rng, n, byte_set):
    """int64 keys whose ordered words differ in exactly the bytes of byte_set (the other bytes are one constant pattern)."""
    base = np.frombuffer(rng.bytes(8), np.uint8).copy()
    raw = np.tile(base, (n, 1))
    for b in byte_set:
        choices = np.array([0x00, 0x80, 0x7f, 0xff] if b == 7 else rng.choice(256, 2 if len(byte_set) > 4 else 4, replace=False), np.uint8)
        raw[:, b] = choices[rng.integers(0, len(choices), n)]
        raw[:len(choices), b] = choices  # every choice occurs
    return raw.view("<i8").reshape(n)


DIGIT_SETS = [(), (0,), (7,), (0, 5), (1, 3, 6), (0, 1, 2, 3, 4, 5, 6, 7)]


@pytest.mark.parametrize("byte_set", DIGIT_SETS, ids=lambda s: "bytes_" + ("".join(map(str, s)) or "none"))
def test_digit_selection_int64(G, byte_set):
    """A pass runs for exactly the bytes in which the words differ: non-adjacent bytes, the sign byte alone, none at all."""
    rng = np.random.default_rng(100 + sum(byte_set))
    n = 70_001
    k = _int64_keys_differing_in(rng, n, byte_set)
    words, _ = SG.sortable_words(HostColumn(k))
    assert differing_bytes(words) == set(byte_set)
    if byte_set == (7,):
        assert (k < 0).any() and (k >= 0).any()
    v = HostColumn(np.arange(n, dtype=np.int32))
    picks = [{"kind": "nth_element", "n": 0}, {"kind": "nth_element", "n": -1}, {"kind": "nth_element", "n": 3}, "count_all"]
    check_call(G, [HostColumn(k)], [(v, picks)], expect={"sort_scatter": len(byte_set), "sort_hist": len(byte_set), "sort_words": 1})
    check_call(G, [HostColumn(k)], [(v, [{"kind": "median"}, {"kind": "nunique"}])])


@pytest.mark.parametrize("key_type,passes", [("uint8", 1), ("int16", 8), ("uint16", 2), ("int8", 8)])
def test_digit_selection_narrow_keys(G, key_type, passes):
    """(A signed narrow key of both signs differs in every byte of its sign-extended word.)"""
    rng = np.random.default_rng(7)
    n = 70_001
    info = np.iinfo(key_type)
    k = rng.integers(info.min, info.max, n, endpoint=True).astype(key_type)
    words, _ = SG.sortable_words(HostColumn(k))
    assert len(differing_bytes(words)) == passes
    v = HostColumn(np.arange(n, dtype=np.int32))
    check_call(G, [HostColumn(k)], [(v, [{"kind": "nth_element", "n": 0}, {"kind": "nth_element", "n": -1}, "count_all"])],
               expect={"sort_scatter": passes})


@pytest.mark.parametrize("nulls", ["some", "none_under_a_mask", "all"])
@pytest.mark.parametrize("include", [False, True], ids=["exclude", "include"])
def test_null_flag_pass_of_a_nullable_key(G, nulls, include):
    """The null flags of a key column are one more pass where both flags occur and none where they do not; dropping the rows of null keys
    is one more again."""
    rng = np.random.default_rng(12)
    n = 70_001
    k = _int64_keys_differing_in(rng, n, (0, 5))
    valid = {"some": rng.random(n) > 0.1, "none_under_a_mask": np.ones(n, bool), "all": np.zeros(n, bool)}[nulls]
    key = HostColumn(k, valid)
    words, _ = SG.sortable_words(key)
    value_passes = len(differing_bytes(words))  # (a null's word is 0: with nulls, every byte the values set differs)
    flag_passes = 1 if nulls == "some" else 0
    passes = value_passes + flag_passes + (flag_passes if not include else 0)
    v = HostColumn(np.arange(n, dtype=np.int32))
    requests = [(v, [{"kind": "nth_element", "n": 0}, {"kind": "nth_element", "n": -1}, "count_all"])]
    if nulls == "all" and not include:  # nothing left
        (gk, gr), launches = launches_of(lambda: G.groupby([key], requests))
        assert len(gk[0][0]) == 0 and launches.get("sort_scatter", 0) == 0
        return
    (gk, _), _ = check_call(G, [key], requests, include, expect={"sort_scatter": passes})
    if include and nulls != "none_under_a_mask":
        assert not gk[0][1][-1] and gk[0][1][:-1].all()  # the null key is one group, placed last


# ---------------------------------------------------------------- tile and spine edges
EDGE_SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 65_535, 65_536, 65_537, 69_633, 4_194_303, 4_194_305, 8_388_609]
EDGE_CASES = [(n, s) for n in EDGE_SIZES for s in ("one", "distinct", "skewed") if n < 4_000_000 or s == "skewed"]


@pytest.mark.parametrize("n,shape", EDGE_CASES, ids=[f"{n}-{s}" for n, s in EDGE_CASES])
def test_tile_and_spine_edges(G, n, shape):
    """Sizes around a wave (64), a sort / scan tile (4096), the one-tile histogram scan (16 radix tiles = 65,536 rows, 17 = 69,633)
    and the second turn of the scan spine (1024 scan tiles = 4,194,304 entries); one group, every row its own group, and one group over
    many tiles next to groups of one and two rows; 15 % nulls among the values, whole groups of them and on the groups' edges."""
    rng = np.random.default_rng(n % 1000 + len(shape))
    k = R.shaped_keys(rng, n, shape)
    v = HostColumn(rng.integers(-1000, 1000, n).astype(np.int64), R.nulls_on_group_edges(rng, k))
    requests = [(v, [{"kind": "median"}, {"kind": "nunique"}, {"kind": "nth_element", "n": 0},
                     {"kind": "nth_element", "n": -1, "null_policy": "exclude"}, "count_all"])]
    check_call(G, [HostColumn(k)], requests, expect={"sort_words": 3})


# ---------------------------------------------------------------- stability
STABILITY_N = 1_000_003
STABILITY_KEYS = {"constant_over_a_tile": lambda rng, i: i // 4096, "two_alternating": lambda rng, i: i % 2, "ascending": lambda rng, i: i,
                  "descending": lambda rng, i: STABILITY_N - i, "three_values": lambda rng, i: rng.integers(0, 3, len(i))}


@pytest.mark.parametrize("shape", list(STABILITY_KEYS))
def test_equal_keys_keep_their_input_order(G, shape):
    """Every lane of a wave on one digit, two digits in turn, nothing to move, everything to move: the n-th row of a group is its n-th
    row in input order (numpy's stable argsort), or null where the group is shorter than |n|."""
    rng = np.random.default_rng(3)
    n = STABILITY_N
    k = STABILITY_KEYS[shape](rng, np.arange(n, dtype=np.int64)).astype(np.int32)
    ns = [0, 1, 63, 64, -1, -2, 4096, -4097]
    v = HostColumn(np.arange(n, dtype=np.int32))
    (_, gr), _ = check_call(G, [HostColumn(k)], [(v, [{"kind": "nth_element", "n": x} for x in ns])], expect={"sort_words": 1})
    order = np.argsort(k, kind="stable")
    starts = np.flatnonzero(np.append(True, k[order][1:] != k[order][:-1]))
    sizes = np.diff(np.append(starts, n))
    for x, (data, valid, _) in zip(ns, gr[0]):
        at = sizes + x if x < 0 else np.full(len(sizes), x)
        inside = (at >= 0) & (at < sizes)
        assert np.array_equal(np.ones(len(sizes), bool) if valid is None else valid, inside), f"n = {x}"
        assert np.array_equal(data[inside], order[(starts + at)[inside]]), f"n = {x}"


# ---------------------------------------------------------------- null keys
def _keys_with_nulls_in_different_columns(rng, n):
    data = [rng.integers(0, 5, n).astype(t) for t in (np.int32, np.int16, np.int64)]
    which = rng.integers(0, 7, n)  # 0..2: that column is null; 3: the first two; 4: all three; 5, 6: none
    valid = [~((which == c) | ((which == 3) & (c < 2)) | (which == 4)) for c in range(3)]
    return data, valid


@pytest.mark.parametrize("n", [1_009, 100_003])
@pytest.mark.parametrize("include", [False, True], ids=["exclude", "include"])
def test_nulls_in_different_key_columns(G, include, n):
    rng = np.random.default_rng(n)
    data, valid = _keys_with_nulls_in_different_columns(rng, n)
    keys = [HostColumn(d, m) for d, m in zip(data, valid)]
    v = R.random_column(rng, n, "int32", 20, 0.3)
    aggs = [{"kind": "median"}, {"kind": "nunique", "null_policy": "include"}, {"kind": "nth_element", "n": 1, "null_policy": "exclude"},
            {"kind": "nth_element", "n": -3}, {"kind": "nth_element", "n": 100_000}, {"kind": "nth_element", "n": -100_000, "null_policy": "exclude"},
            "count_all"]
    (gk, _), exp = check_call(G, keys, [(v, aggs)], include)
    if not include:
        assert all(c[1] is None or c[1].all() for c in gk)
    # groups of one and two rows, and groups whose values are all null
    sizes = exp.results[0][6][0]
    assert include is False or ((sizes == 1).any() or n > 50_000)
    # one surviving row; one all-null column among the three (INCLUDE: grouped by the other two; EXCLUDE: nothing left)
    only = [HostColumn(d, np.arange(n) == n // 2) for d in data]
    (gk, gr), _ = check_call(G, only, [(v, aggs)], False)
    assert len(gk[0][0]) == 1 and gr[0][6][0].tolist() == [1]
    dead = [keys[0], HostColumn(data[1], np.zeros(n, bool)), keys[2]]
    if include:
        (gk, _), _ = check_call(G, dead, [(v, aggs)], True)
        assert not gk[1][1].any()
        (gk, gr), _ = check_call(G, [dead[1]], [(v, aggs)], True)  # an all-null key column alone: one group
        assert len(gk[0][0]) == 1 and not gk[0][1][0] and gr[0][6][0].tolist() == [n]
    else:
        gk, _ = G.groupby(dead, [(v, aggs)])
        assert len(gk[0][0]) == 0


# ---------------------------------------------------------------- pre-sorted keys
def _runs(rng, n):
    lengths = rng.integers(1, 3000, n // 1000 + 2)
    values = rng.integers(0, 50, len(lengths))
    values[1:][values[1:] == values[:-1]] += 50  # adjacent runs differ; a value recurs in runs far apart; nothing ascends
    k = np.repeat(values, lengths)[:n].astype(np.int32)
    assert len(k) == n
    return k, np.cumsum(np.append(False, k[1:] != k[:-1]))  # the run of every row


def test_presorted_keys_are_grouped_by_runs_without_a_sort(G):
    rng = np.random.default_rng(8)
    n = 1_000_003
    k, run = _runs(rng, n)
    assert len(np.unique(k)) < run[-1] and (np.diff(k.astype(np.int64)) < 0).any()
    v = R.random_column(rng, n, "float64", 5000, 0.1)
    picks = [{"kind": "nth_element", "n": 0}, {"kind": "nth_element", "n": -1, "null_policy": "exclude"}, "count_all"]
    # no sort at all for the kinds that read the key order alone
    (gk, gr), _ = check_call(G, [HostColumn(k)], [(v, picks)], keys_are_sorted=True,
                             expect={"sort_words": 0, "sort_scatter": 0, "sort_hist": 0})
    assert len(gk[0][0]) == run[-1] + 1 and np.array_equal(gk[0][0], k[np.flatnonzero(np.append(True, run[1:] != run[:-1]))])
    # the value order is the only sort of a MEDIAN (expected_launches counts no key pass for pre-sorted keys)
    _, launches = launches_of(lambda: G.groupby([HostColumn(k)], [(v, [{"kind": "median"}])], keys_are_sorted=True))
    words, valid = radix_words(v)
    label_null = (run.astype(np.uint64) << np.uint64(1)) | (~valid).astype(np.uint64)
    assert launches["sort_scatter"] == len(differing_bytes(words)) + len(differing_bytes(label_null)) and launches["sort_words"] == 2
    check_call(G, [HostColumn(k)], [(v, [{"kind": "median"}, {"kind": "nunique"}] + picks)], keys_are_sorted=True, expect={"sort_words": 2})
    # null keys, whole runs of them: kept (INCLUDE), still nothing is sorted again; dropped (EXCLUDE), the call is sorted after all
    key_valid = (run % 9 != 4) & (run % 9 != 5)
    nullable = HostColumn(k, key_valid)
    (gk, _), _ = check_call(G, [nullable], [(v, picks)], True, keys_are_sorted=True, expect={"sort_words": 0, "sort_scatter": 0})
    assert len(gk[0][0]) > len(np.unique(k)) + 1 and not gk[0][1].all()
    (gk, _), _ = check_call(G, [nullable], [(v, picks)], False, keys_are_sorted=True, expect={"sort_words": 1})
    assert np.array_equal(gk[0][0], np.unique(k[key_valid]))


# ---------------------------------------------------------------- sliced columns
@pytest.mark.parametrize("offset", [1, 31, 33])
def test_sliced_keys_and_values(G, offset):
    """Columns that are slices of their buffers (mask offsets off the word boundary) against materialised copies of the same rows."""
    rng = np.random.default_rng(offset)
    n = 70_001
    value_offset = {1: 33, 31: 1, 33: 31}[offset]
    kd, kv = rng.integers(-300, 300, n + offset).astype(np.int64), rng.random(n + offset) > 0.08
    k2 = rng.integers(0, 3, n + offset).astype(np.int16)
    vd, vv = rng.normal(size=n + value_offset), rng.random(n + value_offset) > 0.2
    aggs = [{"kind": "median"}, {"kind": "nunique"}, {"kind": "quantile", "quantiles": [0.25, 0.75]}, "count_valid"]
    picks = [{"kind": "nth_element", "n": 0}, {"kind": "nth_element", "n": -2, "null_policy": "exclude"}]
    sliced = ([HostColumn(kd, kv, "int64", offset), HostColumn(k2, None, "int16", offset)], HostColumn(vd, vv, "float64", value_offset))
    copied = ([HostColumn(kd[offset:], kv[offset:]), HostColumn(k2[offset:])], HostColumn(vd[value_offset:], vv[value_offset:]))
    for include in (False, True):
        for kinds in (aggs, aggs + picks):  # both routes
            (ka, ra), _ = check_call(G, sliced[0], [(sliced[1], kinds)], include)
            (kb, rb), _ = check_call(G, copied[0], [(copied[1], kinds)], include)
            for c, (a, b) in enumerate(zip(ka, kb)):
                assert np.array_equal(a[1], b[1]) and np.array_equal(a[0][a[1]] if a[1] is not None else a[0], b[0][b[1]] if b[1] is not None else b[0])
            for j, (a, b) in enumerate(zip(ra[0], rb[0])):
                ok = np.ones(len(a[0]), bool) if a[1] is None else a[1]
                assert (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1])), f"aggregation {j}"
                assert np.array_equal(a[0][ok], b[0][ok], equal_nan=True), f"aggregation {j}"
