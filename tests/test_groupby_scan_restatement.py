"""The numpy restatement of groupby scan / replace_nulls (tests/scan_restatement.py) against every vector transcribed from the
reference's tests (tests/golden/kat_groupby_scan.json): pins the checker the GPU test relies on. CPU only."""
import numpy as np
import pytest

import scan_golden as GD
import scan_restatement as R

CASES = GD.load_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_matches_golden(case):
    keys, values, spec = GD.inputs(case)
    exp_keys, exp = GD.expected(case)
    if spec["kind"] == "replace_nulls":
        got_keys, cols = R.replace_nulls(keys, [values], [spec["policy"]], case["include_null_keys"], case["keys_are_sorted"])
        got = cols[0]
    else:
        got_keys, res = R.scan(keys, [(values, [spec])], case["include_null_keys"], case["keys_are_sorted"])
        got = res[0][0]
        assert got[2] == exp[2]
    GD.same_column(got_keys[0], exp_keys, "keys")
    GD.same_column(got, exp, "result", exact=not (isinstance(case["kind"], dict) and "percentage" in case["kind"]))


def test_golden_covers_every_source():
    files = {c["source"].split(":")[0].rsplit("/", 1)[-1] for c in CASES}
    assert files == {"sum_scan_tests.cpp", "product_scan_tests.cpp", "min_scan_tests.cpp", "max_scan_tests.cpp",
                     "count_scan_tests.cpp", "rank_scan_tests.cpp", "replace_nulls_tests.cpp"}


def test_min_max_order_of_zeros_and_nan():
    keys = [(np.zeros(6, np.int32), None, "int32")]
    v = (np.array([0.0, -0.0, np.nan, 1.0, -np.inf, -0.0]), None, "float64")
    _, res = R.scan(keys, [(v, ["min", "max"])])
    mn, mx = res[0][0][0], res[0][1][0]
    assert mn.tolist()[:4] == [0.0, 0.0, 0.0, 0.0] and np.signbit(mn[1:4]).all() and not np.signbit(mn[0])  # -0 below +0
    assert mn[4] == -np.inf and mn[5] == -np.inf
    assert mx[0] == 0 and mx[1] == 0 and not np.signbit(mx[:2]).any() and np.isnan(mx[2:]).all()  # NaN above everything
    assert mx[2:].view(np.uint64).tolist() == [0x7FF8000000000000] * 4  # the canonical quiet NaN


def test_rank_methods_on_ties():
    keys = [(np.zeros(5, np.int32), None, "int32")]
    v = (np.array([3, 1, 3, 2, 1], np.int64), None, "int64")
    got = {m: R.scan(keys, [(v, [{"kind": "rank", "method": m}])])[1][0][0][0].tolist()
           for m in ("first", "min", "max", "average", "dense")}
    assert got == {"first": [4, 1, 5, 3, 2], "min": [4, 1, 4, 3, 1], "max": [5, 2, 5, 3, 2],
                   "average": [4.5, 1.5, 4.5, 3.0, 1.5], "dense": [3, 1, 3, 2, 1]}
