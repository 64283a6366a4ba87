"""CPU: the numpy restatement of the row filters (tests/copy_if_restatement.py) is pinned against the hand-transcribed vectors of
tests/golden/kat_stream_compaction.json and kat_unique_count.json, and cross-checked on seeded random tables against independent
formulations: pandas dropna(thresh=) for drop_nulls, numpy boolean indexing for the masks, np.diff run boundaries for unique."""
import numpy as np
import pytest

import copy_if_restatement as R
from oracle.oracle import HostColumn

GOLD = R.load_golden()
SC = GOLD["stream_compaction"]


check_expected, run_case = R.check_expected, R.run_case


CASES = [(k, c) for k in ("apply_boolean_mask", "apply_deletion_mask", "drop_nulls", "drop_nans", "unique") for c in SC[k]]
FNS = {"apply_boolean_mask": R.apply_boolean_mask, "apply_deletion_mask": R.apply_deletion_mask, "drop_nulls": R.drop_nulls,
       "drop_nans": R.drop_nans, "unique": R.unique}


@pytest.mark.parametrize("kind,c", CASES, ids=lambda x: x if isinstance(x, str) else x["name"])
def test_restatement_matches_golden(kind, c):
    cols, call = run_case(kind, c, FNS)
    if "throws" in c:
        with pytest.raises(R.LogicError):
            call()
        return
    check_expected(R.take(cols, call()), c["expect"])


@pytest.mark.parametrize("c", GOLD["unique_count"]["unique_count"], ids=lambda c: c["name"])
def test_restatement_matches_golden_unique_count(c):
    cols = R.host_table(c["input"])
    if c["kind"] == "table":
        got = R.unique_count_table(cols, c["nulls"] == "equal")
    else:
        got = R.unique_count_column(cols[0], c["null_policy"] == "include", c["nan_policy"] == "nan_is_null")
    assert got == c["expect"]


def test_golden_lists_what_it_skipped():
    for g in (SC, GOLD["unique_count"]):
        assert g["skipped"] and all(s["why"] for s in g["skipped"])


def test_unique_count_compares_with_the_input_row_before():
    c = HostColumn(np.array([1, 5, 1], dtype=np.int32), np.array([True, False, True]))
    assert R.unique_count_column(c, False, False) == 2


# ---------------------------------------------------------------- independent formulations
@pytest.mark.parametrize("seed", range(4))
def test_drop_nulls_agrees_with_pandas(seed):
    import pandas as pd
    rng = np.random.default_rng(seed)
    n = 500
    data = [rng.integers(0, 100, n).astype(np.float64) for _ in range(4)]
    valid = [rng.random(n) < p for p in (0.5, 0.8, 0.3)] + [None]  # (the last key has no mask)
    cols = [HostColumn(d, v) for d, v in zip(data, valid)]
    df = pd.DataFrame({i: np.where(v, d, np.nan) if v is not None else d for i, (d, v) in enumerate(zip(data, valid))})
    for keys in ([0], [0, 1, 2], [0, 1, 2, 3], [3, 1]):
        for thr in [None] + list(range(0, len(keys) + 2)):
            got = R.drop_nulls(cols, keys, thr)
            expect = df.dropna(subset=keys, thresh=len(keys) if thr is None else thr).index.to_numpy()
            if not any(cols[k].null_count for k in keys):
                expect = np.arange(n)  # the reference's shortcut: no key has a null -> a copy, whatever the threshold
            assert got.tolist() == expect.tolist(), (keys, thr)


@pytest.mark.parametrize("seed", range(4))
def test_masks_agree_with_numpy_indexing(seed):
    rng = np.random.default_rng(100 + seed)
    n = 777
    col = HostColumn(rng.integers(-9, 9, n).astype(np.int64))
    m, v = rng.random(n) < 0.5, rng.random(n) < 0.8
    mask = HostColumn(m, v, "bool")
    rows = np.arange(n)
    assert R.apply_boolean_mask([col], mask).tolist() == rows[m & v].tolist()
    assert R.apply_deletion_mask([col], mask).tolist() == rows[~m & v].tolist()
    assert R.apply_boolean_mask([col], HostColumn(m, None, "bool")).tolist() == rows[m].tolist()


@pytest.mark.parametrize("seed", range(4))
def test_unique_agrees_with_run_boundaries(seed):
    rng = np.random.default_rng(200 + seed)
    k = np.repeat(rng.integers(0, 50, 300), rng.integers(1, 5, 300)).astype(np.int64)
    cols = [HostColumn(np.arange(len(k), dtype=np.int32)), HostColumn(k)]
    starts = np.concatenate([[0], np.flatnonzero(np.diff(k)) + 1])
    ends = np.concatenate([starts[1:], [len(k)]]) - 1
    assert R.unique(cols, [1], "first").tolist() == starts.tolist()
    assert R.unique(cols, [1], "any").tolist() == starts.tolist()
    assert R.unique(cols, [1], "last").tolist() == ends.tolist()
    assert R.unique(cols, [1], "none").tolist() == starts[starts == ends].tolist()
    assert R.unique_count_table([cols[1]]) == len(starts)
    assert R.unique_count_column(cols[1], True, False) == len(starts)


def test_drop_nans_counts_a_null_as_not_nan():
    f = HostColumn(np.array([np.nan, np.nan, 1.0, np.nan], dtype=np.float32), np.array([True, False, True, True]))
    d = HostColumn(np.array([1.0, np.nan, np.nan, np.nan]))
    assert R.drop_nans([f, d], [0, 1]).tolist() == []
    assert R.drop_nans([f, d], [0, 1], 1).tolist() == [0, 1, 2]
    assert R.drop_nans([f, d], [0]).tolist() == [1, 2]
    with pytest.raises(R.LogicError):
        R.drop_nans([f, HostColumn(np.arange(4, dtype=np.int32))], [0, 1])
    with pytest.raises(IndexError):
        R.drop_nulls([f], [1])
