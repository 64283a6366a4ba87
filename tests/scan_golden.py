"""Loader of tests/golden/kat_groupby_scan.json (groupby scan / replace_nulls vectors transcribed from the reference's tests),
shared by the restatement's own test and the GPU test."""
import json
import os

import numpy as np

import scan_restatement as R

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_groupby_scan.json")


def load_cases():
    with open(PATH) as f:
        return json.load(f)["cases"]


def column(data, valid, type_name, scale=0):
    dt = R.TYPES[type_name][0]
    arr = np.asarray(data, dtype=np.float64 if dt in (np.float32, np.float64) else np.int64).astype(dt)
    v = None if valid is None else np.asarray(valid, dtype=bool)
    return (arr, v, type_name, scale)


def inputs(case):
    """(keys, values, spec) of a case; spec is a scan spec or {"kind": "replace_nulls", "policy": ...}."""
    keys = [column(case["keys"], case["key_valid"], case["key_type"])]
    values = column(case["values"], case["value_valid"], case["value_type"], case.get("scale", 0))
    spec = case["kind"] if isinstance(case["kind"], dict) else {"kind": case["kind"]}
    return keys, values, spec


def expected(case):
    """(keys column, result column) as the case states them."""
    spec = case["kind"] if isinstance(case["kind"], dict) else {"kind": case["kind"]}
    if spec["kind"] == "replace_nulls":
        rtype = case["value_type"]
    else:
        rtype = R.scan_type(case["value_type"], spec["kind"], spec)
    keys = column(case["expect_keys"], case["expect_keys_valid"], case["key_type"])
    res = column(case["expect"], case["expect_valid"], rtype, case.get("scale", 0))
    return keys, res


def same_column(got, exp, what, exact=True):
    """got / exp: (data, valid, ...). Valid rows equal (floats by value, NaN == NaN); validity equal where either has a mask."""
    gd, gv = np.asarray(got[0]), got[1]
    ed, ev = np.asarray(exp[0]), exp[1]
    assert len(gd) == len(ed), f"{what}: {len(gd)} rows, expected {len(ed)}"
    gvalid = np.ones(len(gd), bool) if gv is None else np.asarray(gv, bool)
    evalid = np.ones(len(ed), bool) if ev is None else np.asarray(ev, bool)
    assert np.array_equal(gvalid, evalid), f"{what}: validity {gvalid.astype(int)} != {evalid.astype(int)}"
    a, b = gd[evalid], ed[evalid]
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        a, b = a.astype(np.float64), b.astype(np.float64)
        ok = (a == b) | (np.isnan(a) & np.isnan(b))
        if not exact:
            ok |= np.isclose(a, b, rtol=1e-12, atol=0)
    else:
        ok = a.astype(np.int64) == b.astype(np.int64)
    assert ok.all(), f"{what}: {a[~ok][:8]} != {b[~ok][:8]}"
