"""CPU: the numpy restatement of cudf::filtered_join (tests/filtered_join_restatement.py) is pinned against the hand-transcribed
vectors of tests/golden/kat_semi_anti_join.json, and cross-checked on random inputs against the CPU oracle's inner join: the semi
join is the sorted unique left indices of the inner join, the anti join their complement."""
import numpy as np
import pytest

import filtered_join_restatement as R
from oracle.oracle import HostColumn

GOLD = R.load_golden()
SHAPES = ["one_int32", "one_int64", "one_float64", "int8", "two_columns", "three_columns"]


@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: c["name"])
def test_restatement_matches_golden(c):
    semi, anti = R.semi_anti(R.host_table(c["left"]), R.host_table(c["right"]), c["nulls"] == "equal")
    assert semi.dtype == np.int32 and anti.dtype == np.int32
    assert semi.tolist() == c["semi"]
    assert anti.tolist() == c["anti"]


def test_golden_is_consistent():
    for c in GOLD["cases"]:
        n = len(c["left"]["cols"][0]) - c["left"].get("offset", [0])[0] if c["left"]["cols"] else 0
        assert sorted(c["semi"] + c["anti"]) == list(range(n)), c["name"]
    assert GOLD["invalid_load_factors"]["load_factors"] == [-0.1, 0.0, 1.1]
    assert GOLD["large_extent"]["right_rows"] / GOLD["large_extent"]["load_factor"] > 2**31


def _random_tables(rng, shape, nl, nr):
    """(left, right) HostColumn lists of one key shape, with duplicates and nulls on both sides."""
    def col(n, kind, nulls, universe):
        if kind == "f64":
            pool = np.array([0.0, -0.0, np.nan, 1.5, -2.25, np.inf] + list(rng.normal(size=universe)), dtype=np.float64)
            data = pool[rng.integers(0, len(pool), n)]
        elif kind == "i8":
            data = rng.integers(-128, 128, n).astype(np.int8)
        else:
            data = rng.integers(0, universe, n).astype(np.int64 if kind == "i64" else np.int32)
        valid = rng.random(n) > 0.1 if nulls else None
        return HostColumn(data, valid)
    kinds = {"one_int32": ["i32"], "one_int64": ["i64"], "one_float64": ["f64"], "int8": ["i8"], "two_columns": ["i32", "i64"],
             "three_columns": ["i32", "f64", "i8"]}[shape]
    left = [col(nl, k, True, 40) for k in kinds]
    right = [col(nr, k, True, 40) for k in kinds]
    return left, right


@pytest.mark.parametrize("nulls_equal", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_agrees_with_oracle_inner_join(oracle, shape, nulls_equal):
    rng = np.random.default_rng(SHAPES.index(shape) * 2 + int(nulls_equal))
    left, right = _random_tables(rng, shape, 700, 300)
    semi, anti = R.semi_anti(left, right, nulls_equal)
    li, _ = oracle.join(left, right, nulls_equal=nulls_equal, kind="inner")
    expect = np.unique(li).astype(np.int32)
    assert semi.tolist() == expect.tolist()
    assert anti.tolist() == np.setdiff1d(np.arange(700), expect).astype(np.int32).tolist()
