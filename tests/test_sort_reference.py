"""The fast numpy reference of the sort-based groupby (tests/sort_reference.py) against the pinned restatement
(oracle/sort_groupby.py) at sizes the restatement's per-group loops can take. No GPU: this is what lets the GPU tests trust the
fast reference at sizes where the restatement cannot be run."""
import numpy as np
import pytest

import kat
import sort_reference as R
from oracle import sort_groupby as SG
from oracle.oracle import HostColumn

SORT_KINDS = [{"kind": "nth_element", "n": 0}, {"kind": "nth_element", "n": 1, "null_policy": "exclude"},
              {"kind": "nth_element", "n": -1}, {"kind": "nth_element", "n": -2, "null_policy": "exclude"},
              {"kind": "nth_element", "n": 70}, {"kind": "nth_element", "n": -70, "null_policy": "exclude"},
              {"kind": "nunique"}, {"kind": "nunique", "null_policy": "include"}, {"kind": "median"},
              {"kind": "quantile", "quantiles": [0.0, 0.1, 0.5, 0.9, 1.0]},
              {"kind": "quantile", "quantiles": [0.33], "interpolation": "lower"},
              {"kind": "quantile", "quantiles": [0.33], "interpolation": "higher"},
              {"kind": "quantile", "quantiles": [0.5, 0.37], "interpolation": "midpoint"},
              {"kind": "quantile", "quantiles": [0.5, 0.125], "interpolation": "nearest"},
              {"kind": "quantile", "quantiles": [0.5, 0.125], "interpolation": "nearest_half_up"},
              {"kind": "quantile", "quantiles": [-1.0, 2.0, 0.75], "interpolation": "linear"}]


def same(got, exp):
    """Exactly the restatement's answer: same arithmetic in the same order, so not one ulp apart."""
    assert len(got.keys) == len(exp[0])
    for a, e in zip(got.keys, exp[0]):
        kat.compare_columns(a, e, "keys")
        assert a[0].tobytes() == e[0].tobytes(), "key bits"
    for r, (ga, ea) in enumerate(zip(got.results, exp[1])):
        assert len(ga) == len(ea)
        for j, (a, e) in enumerate(zip(ga, ea)):
            kat.compare_columns(a, e, f"request {r} aggregation {j}")
            av = np.ones(len(a[0]), bool) if a[1] is None else a[1]
            assert np.array_equal(a[0][av], e[0][av], equal_nan=np.asarray(a[0]).dtype.kind == "f"), f"request {r} aggregation {j}: not bit-equal"


@pytest.mark.parametrize("key_types", [("int32",), ("int64",), ("float64",), ("float32", "int8"), ("uint16", "int64", "bool")])
@pytest.mark.parametrize("include", [False, True])
def test_random_columns(key_types, include):
    rng = np.random.default_rng(len(key_types) * 100 + len(key_types[0]) + (7 if include else 0))
    n = 5000
    keys = [R.random_column(rng, n, t, 9 if len(key_types) > 1 else 301, 0.07) for t in key_types]
    requests = [(R.random_column(rng, n, "int64", 50, 0.2), SORT_KINDS + ["count_all", "count_valid"]),
                (R.random_column(rng, n, "float64", 1000, 0.1), SORT_KINDS),
                (R.random_column(rng, n, "int16", 40, 0.0), SORT_KINDS + ["count_valid"])]
    got = R.groupby(keys, requests, include_null_keys=include)
    same(got, SG.groupby(keys, requests, include_null_keys=include))
    # first_rows: the first row of each group in input order holds the returned key
    for k, (data, valid, _) in zip(keys, got.keys):
        assert np.array_equal(k.data[got.first_rows] != 0 if k.data.dtype == np.uint8 and data.dtype == bool else k.data[got.first_rows],
                              data, equal_nan=True)


@pytest.mark.parametrize("vt", ["int8", "uint8", "uint32", "uint64", "int64", "float32", "bool", "timestamp_ms"])
def test_every_value_class(vt):
    rng = np.random.default_rng(23)
    n = 3001
    keys = [R.random_column(rng, n, "int32", 37, 0.05)]
    kinds = SORT_KINDS[:8] if vt == "timestamp_ms" else SORT_KINDS
    for include in (False, True):
        requests = [(R.random_column(rng, n, vt, 23, 0.15), kinds)]
        same(R.groupby(keys, requests, include_null_keys=include), SG.groupby(keys, requests, include_null_keys=include))


@pytest.mark.parametrize("shape", ["one", "distinct", "skewed"])
@pytest.mark.parametrize("n", [1, 2, 65, 4097])
def test_shaped_keys_with_nulls_on_group_edges(shape, n):
    rng = np.random.default_rng(n)
    k = R.shaped_keys(rng, n, shape)
    v = HostColumn(rng.integers(-50, 50, n).astype(np.int64), R.nulls_on_group_edges(rng, k))
    requests = [(v, SORT_KINDS + ["count_all"])]
    same(R.groupby([HostColumn(k)], requests), SG.groupby([HostColumn(k)], requests))
    if shape == "skewed" and n == 4097:
        sizes = np.bincount(np.unique(k, return_inverse=True)[1])
        assert sizes.max() >= n // 2 and (sizes == 1).any() and (sizes == 2).any()
        counts = R.groupby([HostColumn(k)], [(v, ["count_valid"])]).results[0][0][0]
        assert (counts == 0).any(), "no group is entirely null"


@pytest.mark.parametrize("include", [False, True])
def test_keys_are_sorted_groups_are_the_runs(include):
    rng = np.random.default_rng(2)
    runs = np.array([5, 3, 9, 3, 1, 5, 5, 2], np.int32)
    k = np.repeat(runs, [40, 1, 70, 2, 300, 1, 2, 64])[:-1]
    n = len(k)
    v = R.random_column(rng, n, "float64", 30, 0.2)
    for kv in (None, rng.random(n) > 0.1):
        keys = [HostColumn(k, kv)]
        got = R.groupby(keys, [(v, SORT_KINDS)], include_null_keys=include, keys_are_sorted=True)
        same(got, SG.groupby(keys, [(v, SORT_KINDS)], include_null_keys=include, keys_are_sorted=True))
        if kv is None:
            assert list(got.keys[0][0]) == [5, 3, 9, 3, 1, 5, 2]  # (two adjacent runs of 5 are one group)
            assert list(got.first_rows) == [0, 40, 41, 111, 113, 413, 416]


def test_null_keys_in_different_columns():
    rng = np.random.default_rng(4)
    n = 2000
    data = [rng.integers(0, 4, n).astype(t) for t in (np.int32, np.int16, np.int64)]
    which = rng.integers(0, 6, n)  # rows 0..2: that column null; 3: the first two; 4, 5: none
    valid = [~((which == c) | ((which == 3) & (c < 2))) for c in range(3)]
    keys = [HostColumn(d, v) for d, v in zip(data, valid)]
    v = R.random_column(rng, n, "int32", 20, 0.3)
    for include in (False, True):
        same(R.groupby(keys, [(v, SORT_KINDS)], include_null_keys=include), SG.groupby(keys, [(v, SORT_KINDS)], include_null_keys=include))
    # all rows but one carry a null somewhere; an all-null column under INCLUDE; nothing left under EXCLUDE
    one = [HostColumn(d, np.arange(n) == 777) for d in data]
    same(R.groupby(one, [(v, SORT_KINDS)]), SG.groupby(one, [(v, SORT_KINDS)]))
    assert len(R.groupby(one, [(v, SORT_KINDS)]).first_rows) == 1
    none = [HostColumn(data[0], np.zeros(n, bool))]
    for include in (False, True):
        same(R.groupby(none, [(v, SORT_KINDS)], include_null_keys=include), SG.groupby(none, [(v, SORT_KINDS)], include_null_keys=include))


def test_sliced_columns():
    rng = np.random.default_rng(6)
    n = 1500
    for offset in (1, 31, 33):
        k = HostColumn(rng.integers(0, 40, n + offset).astype(np.int32), rng.random(n + offset) > 0.1, "int32", offset)
        v = HostColumn(rng.normal(size=n + offset), rng.random(n + offset) > 0.2, "float64", offset)
        same(R.groupby([k], [(v, SORT_KINDS)], include_null_keys=True), SG.groupby([k], [(v, SORT_KINDS)], include_null_keys=True))


def test_int64_midpoint_keeps_halves_and_remainders_apart():
    lim = np.iinfo(np.int64)
    v = np.array([lim.max, lim.max - 2, lim.min, lim.min + 1, -3, -1, -3, 4, 7, 7], np.int64)
    k = np.repeat(np.arange(5, dtype=np.int32), 2)
    req = [(HostColumn(v), [{"kind": "quantile", "quantiles": [0.5], "interpolation": "midpoint"}])]
    got = R.groupby([HostColumn(k)], req)
    same(got, SG.groupby([HostColumn(k)], req))
    assert got.results[0][0][0].tolist() == [float(lim.max - 1), float(lim.min) + 0.0, -2.0, 0.5, 7.0]


def test_empty_input():
    k, v = HostColumn(np.zeros(0, np.int32)), HostColumn(np.zeros(0, np.float64))
    got = R.groupby([k], [(v, SORT_KINDS)])
    assert len(got.keys[0][0]) == 0 and all(len(c[0]) == 0 for c in got.results[0]) and len(got.first_rows) == 0
