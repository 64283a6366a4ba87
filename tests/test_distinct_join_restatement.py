"""CPU: the numpy restatement of cudf::distinct_hash_join (tests/distinct_join_restatement.py) is pinned against the hand-transcribed
vectors of tests/golden/kat_distinct_join.json (which checks the transcription of the reference's gold tables into index vectors),
and cross-checked on random inputs with a distinct build side against the CPU oracle's inner and left joins."""
import numpy as np
import pytest

import distinct_join_restatement as R
from oracle.oracle import HostColumn

GOLD = R.load_golden()
SHAPES = ["one_int32", "one_int64", "one_float64", "three_columns"]


@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: c["name"])
def test_restatement_matches_golden(c):
    left, right = R.case_tables(c)
    eq = c["nulls"] == "equal"
    expect = R.case_expected(c)
    assert expect, c["name"]
    if "inner" in expect:
        li, ri = R.inner(left, right, eq)
        assert li.dtype == np.int32 and ri.dtype == np.int32
        assert li.tolist() == expect["inner"][0].tolist() and ri.tolist() == expect["inner"][1].tolist()
    if "left_join" in expect:
        r = R.right_of_left(left, right, eq)
        assert r.dtype == np.int32 and r.tolist() == expect["left_join"].tolist()


def test_golden_is_consistent():
    for c in GOLD["cases"]:
        e = R.case_expected(c)
        if "inner" in e and "left_join" in e:  # the two statements of one case name the same pairs
            hit = e["left_join"] != R.JoinNoMatch
            assert np.flatnonzero(hit).tolist() == e["inner"][0].tolist() and e["left_join"][hit].tolist() == e["inner"][1].tolist()
        right = R.case_tables(c)[1]
        assert R.distinct_rows(right)[0].size == right[0].size, c["name"]  # the build side is distinct, as the class requires
    assert GOLD["invalid_load_factors"]["load_factors"] == [-0.1, 0.0, 1.1]
    assert GOLD["large_extent"]["right_rows"] / GOLD["large_extent"]["load_factor"] > 2**31
    assert [c["load_factors"] for c in GOLD["cases"] if c["name"] == "PrimitiveInnerJoinWithNulls"] == [[0.5, 1.0]]


def _random_tables(rng, shape, nl, nr):
    """(left, right) HostColumn lists of one key shape with nulls on both sides; the right side made distinct."""
    def col(n, kind, universe):
        if kind == "f64":
            pool = np.array([0.0, -0.0, np.nan, -np.nan, 1.5, -2.25, np.inf] + list(rng.normal(size=universe)), dtype=np.float64)
            data = pool[rng.integers(0, len(pool), n)]
        elif kind == "i8":
            data = rng.integers(-4, 4, n).astype(np.int8)
        else:
            data = rng.integers(0, universe, n).astype(np.int64 if kind == "i64" else np.int32)
        return HostColumn(data, rng.random(n) > 0.1)
    kinds = {"one_int32": ["i32"], "one_int64": ["i64"], "one_float64": ["f64"], "three_columns": ["i32", "f64", "i8"]}[shape]
    universe = 400 if len(kinds) == 1 else 6
    left = [col(nl, k, universe) for k in kinds]
    right = R.distinct_rows([col(nr, k, universe) for k in kinds])
    return left, right


@pytest.mark.parametrize("nulls_equal", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_agrees_with_oracle_joins(oracle, shape, nulls_equal):
    rng = np.random.default_rng(SHAPES.index(shape) * 2 + int(nulls_equal))
    left, right = _random_tables(rng, shape, 700, 300)
    nr = right[0].size
    assert 1 < nr <= 300 and R.distinct_rows(right)[0].size == nr
    li, ri = R.inner(left, right, nulls_equal)
    assert 0 < len(li) < 700
    assert np.all(np.diff(li) > 0)
    ol, orr = oracle.join(left, right, nulls_equal=nulls_equal, kind="inner")
    assert set(zip(li.tolist(), ri.tolist())) == set(zip(ol.tolist(), orr.tolist())) and len(ol) == len(li)
    # the oracle's left join: one pair per left row (the build side is distinct), the unmatched ones with JoinNoMatch
    ol, orr = oracle.join(left, right, nulls_equal=nulls_equal, kind="left")
    assert sorted(ol.tolist()) == list(range(700))
    by_left = np.empty(700, dtype=np.int32)
    by_left[ol] = orr
    assert R.right_of_left(left, right, nulls_equal).tolist() == by_left.tolist()
