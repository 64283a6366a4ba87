"""CPU: the numpy restatement of cudf::rank (tests/rank_restatement.py) against the golden vectors (tests/golden/kat_rank.json) for
every numeric type but bool, and against pandas Series.rank on seeded random int64 and float64 columns, exactly. The pandas
columns hold no NaN, which pandas reads as missing."""
import numpy as np
import pytest

import rank_restatement as R
import sorting_restatement as S
from oracle.oracle import HostColumn

GOLD = R.load_golden()
NUMERIC = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64"]  # (bool: rank_test.cpp:74)
CASES = list(R.golden_cases(GOLD))


def _check(got, expect_values, expect_valid, dtype):
    values, valid = got
    assert values.dtype == dtype
    if expect_valid is None:
        assert valid is None
        assert values.tolist() == list(expect_values)
    else:
        keep = np.array(expect_valid, dtype=bool)
        assert valid.tolist() == keep.tolist()
        assert values[keep].tolist() == np.array(expect_values, dtype=dtype)[keep].tolist()


def test_golden_file_is_complete():
    names = [c["name"] for c in GOLD["cases"]]
    assert len(names) == 36 and len(set(names)) == 36
    plain = {(m, o, na) for m in R.METHODS for o in ("asc", "desc") for na in ("keep", "top", "bottom")}
    assert {(c["method"], c["order"], c["na_option"]) for c in GOLD["cases"] if not c["percentage"]} == plain
    assert sum(1 for c in GOLD["cases"] if c["percentage"]) == 6


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_golden_cases(case):
    _, col, method, order, policy, null_order, pct, values, valid = case
    dtype = np.float64 if pct or method == "average" else np.int32
    for ty in NUMERIC:
        _check(R.rank(R.golden_column(GOLD, col, ty), method, order, policy, null_order, pct), values, valid, dtype)


def test_golden_large():
    g = GOLD["large"]
    got, valid = R.rank(HostColumn(np.arange(g["rows"], dtype=np.int64)), g["method"], g["order"], g["policy"], g["null_order"], False)
    assert valid is None and got.dtype == np.float64 and got.tolist() == [float(i + 1) for i in range(g["rows"])]


@pytest.mark.parametrize("d", GOLD["documented"], ids=lambda d: d["name"])
def test_documented_examples(d):
    col = S.host_column("int32", d["values"], d.get("valid"))
    for method, expect in d["expect"].items():
        keep = d.get("valid") if d["policy"] == "exclude" else None
        _check(R.rank(col, method, "asc", d["policy"], d["null_order"], False), expect, keep,
               np.float64 if method == "average" else np.int32)


PANDAS_NA = {"keep": "keep", "top": "top", "bottom": "bottom"}


@pytest.mark.parametrize("kind", ["int64", "float64"])
@pytest.mark.parametrize("seed", range(3))
def test_agrees_with_pandas(kind, seed):
    import pandas as pd
    rng = np.random.default_rng(100 + seed)
    for n in (1, 2, 7, 50, 333):
        data = rng.integers(-3, 4, n).astype(np.int64)
        if kind == "float64":
            data = data / 2.0  # (halves, both signs, and both zeros below)
            data[rng.random(n) < 0.1] = -0.0
        valid = rng.random(n) < 0.8
        for with_nulls in (False, True):
            col = HostColumn(data, valid if with_nulls else None)
            series = pd.Series(data.astype(np.float64)).where(valid) if with_nulls else pd.Series(data)
            for method in R.METHODS:
                for order in ("asc", "desc"):
                    for na in ("keep", "top", "bottom"):
                        for pct in (False, True):
                            policy, null_order = R.NA_OPTION[na][order]
                            got, got_valid = R.rank(col, method, order, policy, null_order, pct)
                            exp = series.rank(method=method, ascending=order == "asc", na_option=PANDAS_NA[na], pct=pct).to_numpy()
                            keep = np.ones(n, dtype=bool) if got_valid is None else got_valid
                            assert keep.tolist() == (~np.isnan(exp)).tolist()
                            assert got[keep].astype(np.float64).tolist() == exp[keep].tolist(), (n, method, order, na, pct)


def test_ties_are_word_equality():
    """NaNs of any bit pattern tie, -0 ties with +0, nulls tie with each other and with no value - not even with the type's
    lowest, whose value code is 0 like a null's."""
    nan2 = np.array([np.nan], dtype=np.float64).view(np.uint64) | np.uint64(0x8000000000000005)
    f = np.array([0.0, -0.0, np.nan, nan2.view(np.float64)[0], 1.0, np.nan], dtype=np.float64)
    got, _ = R.rank(HostColumn(f), "dense", "asc", "include", "after")
    assert got.tolist() == [1, 1, 3, 3, 2, 3]
    lowest = np.array([-128, 5, -128, 7], dtype=np.int8)
    got, _ = R.rank(HostColumn(lowest, np.array([True, False, False, True])), "min", "asc", "include", "before")
    assert got.tolist() == [3, 1, 1, 4]

