"""TEST INFRASTRUCTURE ONLY - a vectorised numpy statement of the sort-based groupby, for the sizes at which the pinned restatement
(oracle/sort_groupby.py, one Python loop per group) is too slow. Same operation, same result shapes: np.lexsort on
oracle.sort_groupby.sortable_words for the key order (stable, ascending, nulls after, rows of excluded null keys dropped),
np.add.reduceat and index arithmetic per group, quantile interpolation in float64. tests/test_sort_reference.py holds it to the
restatement at small sizes; it reads nothing of the product.

groupby() returns Result(keys, results, first_rows): keys and results in the shapes of oracle.sort_groupby.groupby (so
kat.compare_columns applies), first_rows[g] = the first row of group g in input order - the row whose key the reference returns
(its sort is stable), which lets a test compare key BITS (-0.0 against 0.0, one NaN payload against another).

Kinds: nth_element, nunique, median, quantile, and of the hash kinds count_all and count_valid.
"""
import collections

import numpy as np

from oracle import oracle as O
from oracle import sort_groupby as SG

Result = collections.namedtuple("Result", "keys results first_rows")


class Groups:
    """order (position in key order -> row), offsets (G + 1), labels (per position)."""

    def __init__(self, keys, include_null_keys=False, keys_are_sorted=False):
        self.keys = [SG._as_host(k) for k in keys]
        n = self.keys[0].size
        per_col = [SG.sortable_words(k) for k in self.keys]
        any_null = np.zeros(n, bool)
        for _, valid in per_col:
            any_null |= ~valid
        dropped = int(any_null.sum()) if not include_null_keys else 0
        if keys_are_sorted and not dropped:
            order = np.arange(n, dtype=np.int64)
        else:
            sort_keys = []  # np.lexsort is stable and its LAST key is the primary one
            for (words, valid), k in zip(reversed(per_col), reversed(self.keys)):
                sort_keys.append(words)
                if k.valid is not None:
                    sort_keys.append(~valid)
            if dropped:
                sort_keys.append(any_null)
            order = (np.argsort(sort_keys[0], kind="stable") if len(sort_keys) == 1 else np.lexsort(sort_keys)).astype(np.int64)
        self.num_keys = n - dropped
        self.order = order[:self.num_keys]
        boundary = np.zeros(self.num_keys, bool)
        if self.num_keys:
            boundary[0] = True
        for words, valid in per_col:
            w, v = words[self.order], valid[self.order]
            boundary[1:] |= (w[1:] != w[:-1]) | (v[1:] != v[:-1])
        starts = np.flatnonzero(boundary)
        self.num_groups = len(starts)
        self.offsets = np.append(starts, self.num_keys).astype(np.int64)
        self.labels = np.cumsum(boundary) - 1
        self.sizes = np.diff(self.offsets)

    def first_rows(self):
        return self.order[self.offsets[:-1]]

    def unique_keys(self):
        first = self.first_rows()
        out = []
        for k in self.keys:
            data = k.data[k.offset:k.offset + k.size][first]
            valid = None if k.valid is None else k.valid[k.offset:k.offset + k.size][first]
            if k.type_id == O.TYPE_ID["bool"]:
                data = data != 0
            out.append((data.astype(O.NP_OF_TYPE_ID[k.type_id]), valid, k.type_id))
        return out

    def value_order(self, words, valid):
        """Rows in (label, null, value) order: the valid rows lead each group, ascending."""
        w, v = words[self.order], valid[self.order]
        return self.order[np.lexsort([w, self.labels * 2 + ~v])]

    def per_group_sum(self, per_position):
        """Sum of a per-position array over each group (every group holds at least one position)."""
        if self.num_groups == 0:
            return np.zeros(0, np.int64)
        return np.add.reduceat(per_position.astype(np.int64), self.offsets[:-1])


def _trunc_half(a):
    """a / 2 and a % 2 as C++ computes them (toward zero), without leaving int64."""
    half = (a >> 1) + ((a < 0) & ((a & 1) == 1))
    return half, a - 2 * half


def _quantiles(g, data, valid, vorder, counts, is_int64, qs, interp):
    """quantiles_util.hpp:20-176 for every (group, quantile) at once; doubles throughout."""
    G, nq = g.num_groups, len(qs)
    out, ok = np.zeros(G * nq, np.float64), np.zeros(G * nq, bool)
    live = counts > 0
    c = np.where(live, counts, 1)
    first = g.offsets[:-1]
    as_double = lambda rows: data[rows].astype(np.float64)
    for t, q in enumerate(qs):
        q = min(max(float(q), 0.0), 1.0)
        pos = q * (c - 1).astype(np.float64)
        lower, higher = np.floor(pos).astype(np.int64), np.ceil(pos).astype(np.int64)
        lo_rows, hi_rows = vorder[first + lower], vorder[first + higher]
        if interp == 1:
            r = as_double(lo_rows)
        elif interp == 2:
            r = as_double(hi_rows)
        elif interp == 4:
            r = as_double(vorder[first + np.rint(pos).astype(np.int64)])  # half to even (nearbyint)
        elif interp == 5:
            r = as_double(vorder[first + np.floor(pos + 0.5).astype(np.int64)])  # half away from zero (round), pos >= 0
        elif interp == 3:
            if is_int64:  # quantiles_util.hpp:46-53: halves and remainders apart
                lh, lr = _trunc_half(data[lo_rows].astype(np.int64))
                hh, hr = _trunc_half(data[hi_rows].astype(np.int64))
                r = (lh + hh).astype(np.float64) + (lr + hr).astype(np.float64) * 0.5
            else:
                r = as_double(lo_rows) / 2 + as_double(hi_rows) / 2
        else:
            fraction = pos - lower
            with np.errstate(invalid="ignore"):  # (0 * inf)
                r = (1.0 - fraction) * as_double(lo_rows) + fraction * as_double(hi_rows)
        out[t::nq] = np.where(live, r, 0.0)
        ok[t::nq] = live
    return out, ok


def groupby(keys, requests, include_null_keys=False, keys_are_sorted=False, groups=None):
    """groups: the Groups of the same keys and policies, where a caller already holds them."""
    requests = [(SG._as_host(v), [SG._spec(a) for a in aggs]) for v, aggs in requests]
    g = groups if groups is not None else Groups(keys, include_null_keys, keys_are_sorted)
    G = g.num_groups
    first = g.offsets[:-1]
    results = []
    for v, aggs in requests:
        data, valid = SG._logical(v)
        words = None
        vorder = None
        valid_in_order = valid[g.order]
        counts = g.per_group_sum(valid_in_order)  # valid rows per group
        out = []
        for a in aggs:
            kind = a["kind"]
            tid = SG._result_type(v.type_id, kind)
            npt = O.NP_OF_TYPE_ID[tid]
            if kind in ("median", "quantile", "nunique") and vorder is None:
                words, _ = SG.sortable_words(v)
                vorder = g.value_order(words, valid)
            if kind == "count_all":
                out.append((g.sizes.astype(np.int32), None, tid))
            elif kind == "count_valid":
                out.append((counts.astype(np.int32), None, tid))
            elif kind == "nth_element":
                nth, include = int(a.get("n", 0)), a.get("null_policy", "include") == "include"
                if include or valid.all():
                    size = g.sizes
                    k = size + nth if nth < 0 else np.full(G, nth, np.int64)
                    inside = (k >= 0) & (k < size)
                    rows = g.order[np.where(inside, first + k, 0)] if G else np.zeros(0, np.int64)
                else:  # group_nth_element.cu:73-116: the n-th VALID row of the group, in key order
                    valid_positions = np.flatnonzero(valid_in_order)
                    before = np.cumsum(valid_in_order) - valid_in_order  # valid rows before each position
                    base = before[first] if G else np.zeros(0, np.int64)
                    k = counts + nth if nth < 0 else np.full(G, nth, np.int64)
                    inside = (k >= 0) & (k < counts)
                    rows = g.order[valid_positions[np.where(inside, base + k, 0)]] if inside.any() else np.zeros(G, np.int64)
                ok = inside & valid[rows]
                d = np.where(inside, data[rows], np.zeros(1, data.dtype)).astype(npt)
                out.append((d, None if ok.all() else ok, tid))
            elif kind == "nunique":
                include = a.get("null_policy", "exclude") == "include"
                w, ok = words[vorder], valid[vorder]
                starts = np.zeros(g.num_keys, bool)
                starts[first] = True
                starts[1:] |= w[1:] != w[:-1]
                distinct = g.per_group_sum(starts & ok)
                if include:
                    distinct = distinct + (counts < g.sizes)
                out.append((distinct.astype(np.int32), None, tid))
            elif kind in ("median", "quantile"):
                if v.type_id not in SG._ARITHMETIC_IDS:
                    raise O.OracleError(1, "Only arithmetic types are supported in quantiles")
                qs = [0.5] if kind == "median" else list(a["quantiles"])
                interp = 0 if kind == "median" else SG.INTERPOLATION[a.get("interpolation", "linear")]
                d, ok = _quantiles(g, data, valid, vorder, counts, v.type_id == O.TYPE_ID["int64"], qs, interp)
                out.append((d, ok, tid))  # the reference always allocates the mask (group_quantiles.cu:84-88)
            else:
                raise NotImplementedError(kind)
        results.append(out)
    return Result(g.unique_keys(), results, g.first_rows())


# ---------------------------------------------------------------- input generators shared by the CPU and the GPU tests
def random_column(rng, n, type_name, distinct, null_share):
    """n draws from a pool of `distinct` values that holds the type's limits (floats: NaN twice, both zeros, both infinities)."""
    npt = O.NP_OF_TYPE_ID[O.TYPE_ID[type_name]]
    if np.dtype(npt).kind == "f":
        pool = rng.normal(size=distinct).astype(npt)
        special = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, np.nan], npt)
        pool[: min(len(special), distinct)] = special[: min(len(special), distinct)]
    elif np.dtype(npt).kind == "b":
        pool = np.array([False, True])
    else:
        info = np.iinfo(npt)
        pool = rng.integers(info.min, info.max, size=distinct, dtype=np.int64 if np.dtype(npt).kind == "i" else np.uint64,
                            endpoint=True).astype(npt)
        pool[: min(2, distinct)] = np.array([info.min, info.max], npt)[: min(2, distinct)]
    data = pool[rng.integers(0, len(pool), n)]
    valid = None if null_share == 0 else rng.random(n) >= null_share
    return O.HostColumn(data, valid, type_name)


def shaped_keys(rng, n, shape):
    """int32 keys of n rows. "one": one group; "distinct": a permutation, every row its own group; "skewed": about n / 100 groups -
    one holds half of the rows (many sort tiles at the larger sizes), a third of the others hold 1 or 2 rows - in shuffled order."""
    if shape == "one":
        return np.full(n, -7, np.int32)
    if shape == "distinct":
        return (rng.permutation(n).astype(np.int64) * 3 - n).astype(np.int32)
    assert shape == "skewed"
    G = max(1, n // 100)
    ids = np.zeros(n, np.int64)
    at = n // 2  # group 0: rows [0, at)
    small = max(0, min(G // 3, (n - at) // 2))
    sizes = np.tile([1, 2], small)[:small]
    ids[at:at + sizes.sum()] = np.repeat(np.arange(1, small + 1), sizes)
    at += int(sizes.sum())
    if G - 1 - small > 0:
        ids[at:] = rng.integers(small + 1, G, n - at)
    ids = ids[rng.permutation(n)]
    return (ids * 5 - 2 * G).astype(np.int32)  # both signs


def nulls_on_group_edges(rng, keys, share=0.15):
    """A validity for a values column next to int keys: every 7th group entirely null, every 5th group null in its first and last
    row (in input order), random nulls up to `share` of the rows elsewhere."""
    n = len(keys)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    starts = np.flatnonzero(np.append(True, ks[1:] != ks[:-1]))
    ends = np.append(starts[1:], n)
    label = np.zeros(n, np.int64)
    label[order] = np.repeat(np.arange(len(starts)), ends - starts)
    valid = rng.random(n) >= share
    if len(starts) > 1:
        valid &= label % 7 != 3
    valid[order[starts[::5]]] = False
    valid[order[ends[::5] - 1]] = False
    return valid
