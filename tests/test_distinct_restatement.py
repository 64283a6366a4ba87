"""CPU: the numpy restatement of cudf::distinct (tests/distinct_restatement.py) is pinned against the hand-transcribed vectors of
tests/golden/kat_distinct.json, and cross-checked on random NaN-free, null-free tables against pandas drop_duplicates."""
import numpy as np
import pytest

import distinct_restatement as R
from oracle.oracle import HostColumn

GOLD = R.load_golden()


def _payload(cols, idx):
    if not cols:
        return []
    c = cols[0]
    return sorted(np.asarray(c.data)[c.offset:c.offset + c.size][idx].tolist())


@pytest.mark.parametrize("c", GOLD["distinct"], ids=lambda c: c["name"])
def test_restatement_matches_golden_distinct(c):
    cols = R.host_table(c["input"])
    if not cols or not c["keys"] or cols[0].size == 0:
        assert c["expect_payload_sorted"] == []
        return
    idx = R.distinct_indices([cols[k] for k in c["keys"]], c["keep"], c["nulls"] == "equal", c["nans"] == "equal")
    assert idx.dtype == np.int32 and np.all(np.diff(idx) > 0)
    assert _payload(cols, idx) == c["expect_payload_sorted"]
    if "expect_indices" in c:
        assert idx.tolist() == c["expect_indices"]


@pytest.mark.parametrize("c", GOLD["stable_distinct"], ids=lambda c: c["name"])
def test_restatement_matches_golden_stable_distinct(c):
    """stable_distinct is the gather at the ascending indices: column 0 in the order the reference pins."""
    cols = R.host_table(c["input"])
    if not cols or not c["keys"] or cols[0].size == 0:
        assert c["expect_payload_in_order"] == []
        return
    idx = R.distinct_indices([cols[k] for k in c["keys"]], c["keep"], c["nulls"] == "equal", c["nans"] == "equal")
    c0 = cols[0]
    assert np.asarray(c0.data)[c0.offset:c0.offset + c0.size][idx].tolist() == c["expect_payload_in_order"]


@pytest.mark.parametrize("c", GOLD["distinct_count"], ids=lambda c: c["name"])
def test_restatement_matches_golden_count(c):
    cols = R.host_table(c["input"])
    if c["kind"] == "table":
        got = R.distinct_count_table(cols, c["nulls"] == "equal")
    else:
        got = R.distinct_count_column(cols[0], c["null_policy"] == "include", c["nan_policy"] == "nan_is_null")
    assert got == c["expect"]


def test_golden_lists_what_it_skipped():
    assert GOLD["skipped"] and all(s["why"] for s in GOLD["skipped"])


SHAPES = [["i64"], ["i32", "i8"], ["f64"], ["i32", "f32", "u16"]]


@pytest.mark.parametrize("keep", ["first", "last", "none"])
@pytest.mark.parametrize("shape", range(len(SHAPES)))
def test_restatement_agrees_with_pandas(shape, keep):
    import pandas as pd
    rng = np.random.default_rng(shape * 3 + ["first", "last", "none"].index(keep))
    n = 2000
    kinds = {"i64": np.int64, "i32": np.int32, "i8": np.int8, "u16": np.uint16, "f64": np.float64, "f32": np.float32}
    data = []
    for k in SHAPES[shape]:
        v = rng.integers(0, 30, n)
        if k.startswith("f"):
            v = np.where(rng.random(n) < 0.1, -0.0, v * 0.5)  # -0 equals +0
        data.append(v.astype(kinds[k]))
    got = R.distinct_indices([HostColumn(d) for d in data], keep)
    df = pd.DataFrame({f"c{i}": d for i, d in enumerate(data)})
    expect = np.flatnonzero(~df.duplicated(keep=False if keep == "none" else keep).to_numpy())
    assert got.tolist() == expect.tolist()
    assert R.distinct_count_table([HostColumn(d) for d in data]) == len(df.drop_duplicates())
