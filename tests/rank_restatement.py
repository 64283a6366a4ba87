"""A numpy restatement of the cudf::rank contract (include/cudf/sorting.hpp; reference cpp/src/sort/rank.cu:253-353): the checker
of the GPU tests. Built on sorting_restatement: the order is its stable sorted_order and two rows tie exactly when their
packed_words are equal, so NaNs tie, -0 ties with +0 and all nulls form one run.

rank(col, method, order, policy, null_order, percentage) -> (values, valid or None)
  method "first" / "average" / "min" / "max" / "dense"; order "asc" / "desc"; policy "include" / "exclude"; null_order "before" /
  "after". values: float64 for "average" or a percentage, else int32. valid: the column's validity under "exclude" when it has a
  mask, else None; the values under a null are unspecified (here: whatever the formulas give).
The only floating-point steps are min + (count - 1) / 2.0 and one division, both correctly rounded in numpy and on the device, so
the GPU tests compare exactly."""
import json
import os

import numpy as np

import sorting_restatement as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_rank.json")
METHODS = ["first", "average", "min", "max", "dense"]
# (order, policy, null_order) where the reference defines the result (sorting.hpp:204-206): "exclude" only with the nulls last
DEFINED = [("asc", "exclude", "after"), ("asc", "include", "before"), ("asc", "include", "after"),
           ("desc", "exclude", "before"), ("desc", "include", "after"), ("desc", "include", "before")]
# the golden file's names for them (rank_test.cpp:47-56: keep / top / bottom are pandas' na_option)
NA_OPTION = {"keep": {"asc": ("exclude", "after"), "desc": ("exclude", "before")},
             "top": {"asc": ("include", "before"), "desc": ("include", "after")},
             "bottom": {"asc": ("include", "after"), "desc": ("include", "before")}}


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def run_flags(col, order, null_order, idx):
    """head[i]: sorted position i starts a run of equal rows."""
    n = len(idx)
    head = np.zeros(n, dtype=bool)
    if n:
        head[0] = True
    for w in S.packed_words([col], [order], [null_order]):
        s = w[idx]
        head[1:] |= s[1:] != s[:-1]
    return head


def rank(col, method, order="asc", policy="exclude", null_order="after", percentage=False):
    assert method in METHODS and order in ("asc", "desc") and policy in ("include", "exclude") and null_order in ("before", "after")
    n = col.size
    dtype = np.float64 if percentage or method == "average" else np.int32
    _, valid = S._rows(col)
    out_valid = valid.copy() if policy == "exclude" and col.valid is not None else None
    if n == 0:  # an empty column of the output type, without a mask
        return np.zeros(0, dtype=dtype), None
    idx = S.sorted_order([col], [order], [null_order]).astype(np.int64)
    head = run_flags(col, order, null_order, idx)
    pos = np.arange(n, dtype=np.int64)
    # forward: the last head at or before i; backward: the first position at or after i whose successor is a head (or the end)
    first = np.maximum.accumulate(np.where(head, pos, 0))
    tail = np.append(head[1:], True)
    last = np.minimum.accumulate(np.where(tail, pos, n)[::-1])[::-1]
    dense = np.cumsum(head)
    if method == "first":
        r = pos + 1
    elif method == "min":
        r = first + 1
    elif method == "max":
        r = last + 1
    elif method == "dense":
        r = dense
    else:  # rank.cu:244-247
        r = (first + 1).astype(np.float64) + ((last - first + 1).astype(np.float64) - 1) / 2.0
    if percentage:
        count = n if policy == "include" else n - col.null_count  # rank.cu:339-340
        with np.errstate(divide="ignore", invalid="ignore"):  # (count == 0: every row is null, no value is compared)
            divisor = (dense[count - 1] if count > 0 else 0) if method == "dense" else count  # rank.cu:349
            r = r.astype(np.float64) / np.float64(divisor)
    out = np.empty(n, dtype=dtype)
    out[idx] = r.astype(dtype)
    return out, out_valid


# ---------------------------------------------------------------- the golden vectors
def golden_cases(gold):
    """(name, input column name, method, order, policy, null_order, percentage, expected values, expected valid or None)."""
    for c in gold["cases"]:
        policy, null_order = NA_OPTION[c["na_option"]][c["order"]]
        for name in ("col1", "col2"):
            exp = c["expect"][name]
            yield (c["name"], name, c["method"], c["order"], policy, null_order, c["percentage"], exp["values"], exp.get("valid"))


def golden_column(gold, name, ty):
    d = gold["inputs"][name]
    return S.host_column(ty, d["values"], d.get("valid"))
