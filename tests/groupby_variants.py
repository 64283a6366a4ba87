"""Which compiled instantiation of the hash-groupby kernels a call must launch, and a table of calls that launches every one.

Three parts, none of which touches the GPU:
  1. a plain restatement of the planner's record layout and accumulator list (csrc/groupby/plan.cpp) and of the three host-side
     dispatch ladders: k_aggregate (aggregate_columns.hip, aggregate_kernel.inl launch_aggregate_records / launch_aggregate_t),
     the exact partition kernels (partition_kernels.hip launch_partition_hist / launch_partition_scatter) and the ring scatter
     (dense_ring_kernels.hip launch_dense_ring_scatter). From the facts of a call they give the labels the library's variant
     registry (_lib.profile_variants) must count for that call;
  2. a generator that builds the input of a call FROM those facts (column types, nullability, aggregation sets, the form the
     planner's switches force) with data that can expose a wrong instantiation;
  3. CASES, chosen greedily from a systematic enumeration of such facts so that every label is launched by some case, and
     UNREACHABLE, the registered labels no input can reach, each with the dispatch condition that rules it out.
tests/test_groupby_variants.py checks the table against the registry on the CPU; tests/test_groupby_variants_gpu.py runs it."""
import itertools

import numpy as np

from oracle.oracle import HostColumn

FAMILIES = ("aggregate", "partition", "ring_scatter")  # the families the case table covers completely


class PlanError(Exception):
    """A documented per-call limit of the planner (the message is the library's)."""


# ------------------------------------------------------------------------------------------------ the plan (plan.cpp)
def _cls(t):
    return "f" if t.startswith("float") else ("u" if t.startswith("uint") else "i")


def _width(t):
    return {"8": 1, "16": 2, "32": 4, "64": 8}[t.lstrip("uintfloa")]


SRC_IDS = {"value": 0, "one_if_valid": 1, "one": 2, "square": 3, "arg_idx": 4, "arg_idx_of_max": 5}


class Plan:
    """keys: [type name]; values: [(type name, has nulls)]; requests: [(value index, [kind])]. Keys carry no nulls here."""

    def __init__(self, keys, values, requests):
        self.keys, self.values, self.requests = list(keys), list(values), [(v, list(k)) for v, k in requests]
        if len(values) > 7:
            raise PlanError("Too many distinct value columns")
        self._accumulators()
        self._units()
        # plan_fast_path: every unit a plain 8-byte column without nulls, no row id
        self.simple = (all(_width(t) == 8 and _cls(t) in "iu" for t in keys) and not self.rowid and
                       all(_width(t) == 8 and not nulls for t, nulls in values))
        self.ncols = len(keys) + len(values)
        self.RU, self.PU = self.KU + self.NPAY, self.KU + self.NACC
        self.slot_bytes = 8 * self.KU + 4 + sum(4 if a[0] == "addi" and a[1] in ("one", "one_if_valid") else 8 for a in self.accs)

    def _accumulators(self):
        accs, self.narg = [], 0

        def add(d):
            if d in accs:
                return
            if len(accs) >= 12:
                raise PlanError("Too many distinct accumulators")
            accs.append(d)
        for vidx, kinds in self.requests:
            t, nulls = self.values[vidx]
            c, vbit = _cls(t), (vidx if nulls else -1)
            s = "f" if c == "f" else "i"

            def count_valid():
                add(("addi", "one_if_valid", vidx, vbit) if nulls else ("addi", "one", -1, -1))
            for k in kinds:
                nullable = nulls
                if k == "sum":
                    add(("add" + s, "value", vidx, vbit))
                elif k == "sum_of_squares":
                    add(("add" + s, "square", vidx, vbit))
                elif k == "product":
                    add(("mul" + s, "value", vidx, vbit))
                elif k in ("min", "max"):
                    add((k + c, "value", vidx, vbit))
                elif k in ("argmin", "argmax"):
                    add((k[3:] + c, "value", vidx, vbit))
                    idx = ("mini", "arg_idx" if k == "argmin" else "arg_idx_of_max", vidx, vbit)
                    if idx not in accs:
                        if len(accs) >= 12:
                            raise PlanError("Too many distinct accumulators")
                        if self.narg >= 4:
                            raise PlanError("Too many ARGMIN / ARGMAX")
                        accs.append(idx)
                        self.narg += 1
                elif k == "count_valid":
                    count_valid()
                    nullable = False
                elif k == "count_all":
                    add(("addi", "one", -1, -1))
                    nullable = False
                elif k == "mean":
                    add(("add" + s, "value", vidx, vbit))
                    count_valid()
                else:
                    raise ValueError(k)
                if nullable:  # the result's validity comes from the count of valid rows
                    count_valid()
        self.accs, self.NACC = accs, len(accs)
        self.rowid = any(k.startswith("arg") for _, kinds in self.requests for k in kinds)

    def _units(self):
        # 8-byte key columns take a unit each, narrower ones share units two per unit; the validity flags of the value columns
        # ride in a free high half of the last key unit, else in the row-id unit, else in a unit of their own
        u = sum(1 for t in self.keys if _width(t) == 8)
        narrow = sum(1 for t in self.keys if _width(t) < 8)
        if u > 4 or (narrow and u + (narrow + 1) // 2 > 4):
            raise PlanError("Key too wide")
        u += narrow // 2
        half = narrow % 2
        need_flags = any(nulls for _, nulls in self.values)
        self.flags_unit = -1
        if need_flags and half:
            self.flags_unit = u
        u += half
        self.KU = u
        u += len(self.values)
        if self.rowid:
            if need_flags and self.flags_unit < 0:
                self.flags_unit = u
            u += 1
        if need_flags and self.flags_unit < 0:
            self.flags_unit = u
            u += 1
        if u > 16:
            raise PlanError("Record too wide")
        self.NPAY = u - self.KU

    def sig(self):
        """device_common.hpp plan_sig spelled as sig_label spells it ("rt": no static encoding)."""
        if not 1 <= self.NACC <= 4 or any(a[2] > 5 or a[3] > 5 or SRC_IDS[a[1]] > 3 for a in self.accs):
            return "rt"
        idx = lambda v: "-" if v < 0 else str(v)
        return "+".join(f"{op}.{src}.p{idx(pay)}.v{idx(vbit)}" for op, src, pay, vbit in self.accs)


SUMF_CNT = "addf.value.p0.v-+addi.one.p-.v-"
SUMI_CNT = "addi.value.p0.v-+addi.one.p-.v-"
SUMF = "addf.value.p0.v-"
SUMI = "addi.value.p0.v-"
CNT = "addi.one.p-.v-"
SUMF_CNT_NULLS = "addf.value.p0.v0+addi.one_if_valid.p0.v0"
SUMI_CNT_NULLS = "addi.value.p0.v0+addi.one_if_valid.p0.v0"
MEAN_MIN_MAX_F_NULLS = SUMF_CNT_NULLS + "+minf.value.p0.v0+maxf.value.p0.v0"
MEAN_MIN_MAX_F = SUMF_CNT + "+minf.value.p0.v-+maxf.value.p0.v-"


# ------------------------------------------------------------------------------------------------ the dispatch ladders
def _agg(inp, kut, payt, nacct, simple, exact, sig="rt"):
    return f"aggregate<{inp},ku{kut},pay{payt},acc{nacct},{'plain' if simple else 'generic'},{'exact' if exact else 'anywidth'},{sig}>"


def _bucket(nacc):  # launch_aggregate_t
    return 2 if nacc <= 2 else (4 if nacc <= 4 else 12)


def aggregate_columns_label(p):
    """aggregate_columns.hip launch_aggregate_columns"""
    sig = p.sig()
    if p.simple and p.KU == 1 and p.NPAY == 1:
        if sig in (SUMF_CNT, SUMI_CNT, SUMF, SUMI):
            return _agg("columns", 1, 1, 2, True, True, sig)
        return _agg("columns", 1, 1, _bucket(p.NACC), True, True)
    if not p.simple and 1 <= p.NPAY <= 2 and 1 <= p.KU <= 2 and p.ncols <= 6:
        if p.KU == 1 and p.NPAY == 1 and sig in (SUMF_CNT, SUMI_CNT, SUMF_CNT_NULLS, SUMI_CNT_NULLS):
            return _agg("columns", 1, 1, 2, False, True, sig)
        if p.KU == 1 and p.NPAY == 2 and sig in (SUMF_CNT_NULLS, SUMI_CNT_NULLS):
            return _agg("columns", 1, 2, 2, False, True, sig)
        return _agg("columns", p.KU, p.NPAY, _bucket(p.NACC), False, True)
    kut = 1 if p.KU <= 1 else (2 if p.KU <= 2 else 4)
    return _agg("columns", kut, 0, _bucket(p.NACC), p.simple, False)


def aggregate_records_label(inp, p):
    """aggregate_kernel.inl launch_aggregate_records<raw | partial>"""
    KU, npay = p.KU, (p.NPAY if inp == "raw" else p.NACC)
    if inp == "raw":
        sig = p.sig()
        if KU == 1 and npay == 1 and p.flags_unit < 0 and sig in (SUMF_CNT, SUMI_CNT, SUMF, SUMI, CNT):
            return _agg(inp, 1, 1, 2, False, True, sig)
        if KU == 1 and npay in (1, 2) and sig in (SUMF_CNT_NULLS, SUMI_CNT_NULLS):
            return _agg(inp, 1, npay, 2, False, True, sig)
        if KU == 2 and npay == 1 and sig == MEAN_MIN_MAX_F_NULLS:
            return _agg(inp, 2, 1, 4, False, True, sig)
        if KU in (1, 2) and npay == 1 and p.flags_unit < 0 and sig == MEAN_MIN_MAX_F:
            return _agg(inp, KU, 1, 4, False, True, sig)
    if (KU, npay) in ((1, 1), (1, 2), (2, 1), (2, 4)):
        return _agg(inp, KU, npay, _bucket(p.NACC), False, True)
    kut = 1 if KU <= 1 else (2 if KU <= 2 else 4)
    return _agg(inp, kut, 0, _bucket(p.NACC), False, False)


def hist_label(simple):
    return f"partition_hist<{'plain' if simple else 'generic'}>"


def scatter_label(units, simple):
    """partition_kernels.hip launch_partition_scatter without write-combining: the next record width with an instantiation"""
    ut = next(c for c in (2, 3, 4, 6, 8, 12, 16) if units <= c)
    rpt = {2: 8, 3: 4, 4: 4, 6: 2, 8: 2, 12: 1, 16: 1}[ut]
    if ut <= 4:
        return f"partition_scatter<ut{ut},rpt{rpt},{'plain' if simple else 'generic'},exact>"
    return f"partition_scatter<ut{ut},rpt{rpt},generic,anywidth>"


# static column shapes of the ring scatter (dense_ring_kernels.hip): (key 0 width, mask, key 1 width or 0, mask, value mask)
RING_SHAPES = [(8, False, 4, True, True), (4, False, 0, False, False), (4, False, 0, False, True), (8, False, 0, False, True),
               (8, False, 4, False, False)]


def _shape_label(w0, m0, w1, m1, mv):
    return f"k{w0}{'m' if m0 else ''}" + (f".k{w1}{'m' if m1 else ''}" if w1 else "") + (".vm" if mv else ".v")


def ring_labels(keys, value, hot, two_level):
    """launch_dense_ring_scatter for keys [(type, has nulls)], the one value column (type, has nulls); two levels: 32-bit tags
    on the first, then the regions level."""
    tag = 32 if two_level else 16
    plain = len(keys) == 1 and keys[0] in (("int64", False), ("uint64", False)) and _width(value[0]) == 8 and not value[1]
    if plain:  # dense_candidate: one plain key column, one plain value column
        first = f"ring_scatter<simple,rpt4,d2,tag{tag},{'hot' if hot else 'nohot'},->"
    else:
        assert not hot
        shape = (_width(keys[0][0]), keys[0][1], _width(keys[1][0]) if len(keys) == 2 else 0, keys[1][1] if len(keys) == 2 else False, value[1])
        if len(keys) <= 2 and _width(value[0]) == 8 and shape in RING_SHAPES:
            wide = shape[2] != 0 and (shape[1] or shape[3])  # two key columns with masks: one tile of loads in flight
            first = f"ring_scatter<static,rpt4,d{1 if wide else 2},tag{tag},nohot,{_shape_label(*shape)}>"
        else:
            first = f"ring_scatter<cols,rpt4,d1,tag{tag},nohot,->"
    return {first} | ({"ring_scatter<regions,rpt4,d2,tag16,nohot,->"} if two_level else set())


# ------------------------------------------------------------------------------------------------ forms: what the switches force
# Sizes are derived from the planner (estimate.cpp, paths_hash.cpp), see each form.
NO_DENSE = {"CUDF_AMD_GB_DENSE": "0", "CUDF_AMD_GB_ARG_LOOKUP": "0"}
SMALL_LDS_KB = 16


def _small_cap(p):
    return min(SMALL_LDS_KB * 1024 // p.slot_bytes, 16384) & ~3


class Case:
    """One call: the plan's facts, the form, and from them the environment, the sizes and the labels it must launch."""

    def __init__(self, name, form, keys, values, requests):
        self.name, self.form, self.plan = name, form, Plan(keys, values, requests)
        p = self.plan
        cols = aggregate_columns_label(p)
        if form == "single":
            # n < 2 * 16384: run_single_pass makes one work item, so no merge round; a few hundred groups fit one table of any plan
            self.env, self.n, self.groups, self.sorted = dict(NO_DENSE), 20_011, 300, False
            self.labels = {cols}
        elif form == "merge":
            # 2 <= n / 16384 < 3: two row chunks, hence one merge launch over their partial records
            self.env, self.n, self.groups, self.sorted = dict(NO_DENSE), 40_009, 300, False
            self.labels = {cols, aggregate_records_label("partial", p)}
        elif form == "partition":
            # 16 KiB tables; n < 2^22 rules the optimistic (write-combining) scatters out, so run_partitioned takes the exact
            # pipeline. Groups: far more than one table holds, few enough that plan_attempt asks for at most ~600 tables (one level:
            # a second level would add the record forms of the histogram and scatter to a plain plan's labels)
            cap = _small_cap(p)
            plan_fill = max(1.0, cap * (0.45 if p.RU in (2, 3) and p.KU == 1 else 0.25))
            self.env, self.n, self.sorted = dict(NO_DENSE, CUDF_AMD_GB_LDS_KB=str(SMALL_LDS_KB)), 150_001, False
            self.groups = min(20_000, int(600 * plan_fill / 1.3))
            self.labels = {hist_label(p.simple), scatter_label(p.RU, p.simple), aggregate_records_label("raw", p)}
        elif form == "sorted":
            # path A (try_preaggregate): rows sorted by key, 16 KiB tables, the table form of the front end. Chunks of 16384 rows
            # must hold fewer keys than a table's fill limit (groups <= 4 x the limit: ~0.45 of it per chunk) while all groups do
            # not fit one table; the chunks' partial records then take the exact pipeline as records of KU + NACC units
            if p.narg:
                raise PlanError("path A takes no ARGMIN / ARGMAX")
            self.env = dict(NO_DENSE, CUDF_AMD_GB_LDS_KB=str(SMALL_LDS_KB), CUDF_AMD_GB_BIG_MIN_ROWS="1000", CUDF_AMD_GB_COLLAPSE_RUNS="0")
            self.n, self.groups, self.sorted = 150_001, 4 * int(_small_cap(p) * 0.6), True
            self.labels = {cols, hist_label(False), scatter_label(p.PU, False), aggregate_records_label("partial", p)}
        else:
            raise ValueError(form)

    def __repr__(self):
        return self.name


def _product_values(rng, n):
    """Factors whose product stays exact over thousands of rows: mostly +-1, a 2, -2 or 3 every few hundred rows."""
    v = rng.choice(np.array([-1, 1], np.int64), n)
    rare = rng.random(n) < 0.002
    v[rare] = rng.choice(np.array([2, -2, 3], np.int64), int(rare.sum()))
    return v


def build_inputs(case):
    """(keys, requests) as HostColumns. Row count no multiple of 64; group sizes from one row to a twentieth of the rows; value
    columns that differ from each other, with negative values; a nullable column has ~20 % nulls and one large group whose
    values are all null; outside the plain path the first value column sits at offset 5 (data and mask)."""
    p, n, G = case.plan, case.n, case.groups
    rng = np.random.default_rng(abs(hash_name(case.name)))
    table = []
    for t in p.keys:
        if _width(t) == 8:
            table.append(rng.integers(-2**62, 2**62, G, dtype=np.int64).astype(t))
        else:
            table.append(rng.integers(-2**31, 2**31 - 1, G, dtype=np.int64).astype(t))
    # every group once, then the other rows skewed towards the first groups (group 0 gets ~G^(-1/3) of them); the last twentieth
    # of the groups stay singletons
    rest = (0.95 * G * rng.random(n - G) ** 3).astype(np.int64)
    assign = rng.permutation(np.concatenate([np.arange(G), rest]))
    if case.sorted:
        order = np.lexsort([c[assign] for c in table][::-1])
        assign = assign[order]
    keys = [HostColumn(c[assign], None, t) for c, t in zip(table, p.keys)]
    cols = []
    for j, (t, nulls) in enumerate(p.values):
        kinds = [k for v, ks in p.requests if v == j for k in ks]
        if "product" in kinds:
            data = _product_values(rng, n).astype(t)
        else:  # (floats: multiples of 0.5, so that sums and sums of squares are exact in any order)
            data = rng.integers(-50 - j, 51 + j, n)
            data = (data * 0.5).astype(t) if _cls(t) == "f" else data.astype(t)
        valid = None
        if nulls:
            valid = (rng.random(n) > 0.2) & (assign != 1)
        offset = 5 if (j == 0 and not p.simple) else 0
        if offset:
            data = np.concatenate([np.full(offset, 77, data.dtype), data])
            valid = None if valid is None else np.concatenate([np.array([True, False, True, True, False]), valid])
        cols.append(HostColumn(data, valid, t, offset=offset))
    return keys, [(cols[v], kinds) for v, kinds in p.requests]


def small_inputs(keys, values, requests, n=1000):
    """A small call of the given shape (for the plans one wider than a limit, which must be refused whatever the data)."""
    rng = np.random.default_rng(7)
    k = [HostColumn(rng.integers(0, 5, n).astype(t), None, t) for t in keys]
    cols = [HostColumn(rng.integers(-9, 10, n).astype(t), (rng.random(n) > 0.2) if nulls else None, t) for t, nulls in values]
    return k, [(cols[v], kinds) for v, kinds in requests]


def hash_name(name):
    h = 1469598103934665603
    for ch in name.encode():
        h = ((h ^ ch) * 1099511628211) % (1 << 63)
    return h


# ------------------------------------------------------------------------------------------------ the systematic enumeration
KEYSETS = [["int64"], ["int32"], ["int64", "int64"], ["int64", "int32"], ["int64", "int64", "int64"],
           ["int64", "int64", "int64", "int32"], ["int64", "int64", "int64", "int64"]]
# aggregation sets of the first value column: the accumulator signatures with an instantiation of their own, then sets whose
# accumulators all hold different numbers and fill the buckets of 2, 4 and 12 accumulators
AGGSETS = {"sum_count": ["sum", "count_all"], "sum": ["sum"], "count": ["count_all"], "sum_valid": ["sum", "count_valid"],
           "mean_min_max": ["mean", "min", "max"], "min": ["min"], "three": ["sum", "min", "max"],
           "six": ["sum", "min", "max", "count_all", "sum_of_squares", "product"], "arg": ["argmin"], "args": ["argmin", "argmax"],
           "args_six": ["argmin", "argmax", "sum", "count_all", "product"]}
FORMS = ("single", "merge", "partition", "sorted")


def _enumerate():
    for keys, t0, nulls, nvals, (aname, aggs), others in itertools.product(KEYSETS, ("int64", "float64", "int32"), (False, True), range(1, 8),
                                                                          AGGSETS.items(), ("sum", "count_all")):
        if nvals == 1 and others != "sum":
            continue
        values = [(t0, nulls)] + [("int64", False)] * (nvals - 1)
        requests = [(0, aggs)] + [(j, [others]) for j in range(1, nvals)]
        name = f"{'_'.join(k.replace('int', 'i') for k in keys)}-{t0.replace('int', 'i').replace('float', 'f')}{'n' if nulls else ''}-{aname}"
        if nvals > 1:
            name += f"-{nvals - 1}x{others}"
        yield name, keys, values, requests


def _greedy_cases():
    covered, cases = set(), []
    for form in FORMS:
        for name, keys, values, requests in _enumerate():
            try:
                c = Case(f"{form}-{name}", form, keys, values, requests)
            except PlanError:
                continue
            if c.labels - covered:
                covered |= c.labels
                cases.append(c)
    return cases


# ---- the plan limits test_fuzz_against_oracle skips around, through single pass and through the exact partition pipeline
_WIDE_KEYS = ["int64", "int64", "int64", "int32"]
_WIDE_VALUES = [("int64", True)] + [("int64", False)] * 5 + [("float64", False)]
_WIDE_REQUESTS = [(0, ["sum", "argmin"]), (1, ["sum"]), (2, ["min"]), (3, ["max"]), (4, ["sum_of_squares"]), (5, ["product"]), (6, ["sum", "argmax"])]
_ARGS_VALUES = [("int64", False), ("float64", False)]
_ARGS_REQUESTS = [(0, ["argmin", "argmax", "sum", "count_all"]), (1, ["argmin", "argmax", "product"])]
LIMIT_CASES = [Case(f"{form}-limit-{name}", form, k, v, r)
               for name, k, v, r in (("widest_record", _WIDE_KEYS, _WIDE_VALUES, _WIDE_REQUESTS), ("eleven_accumulators", ["int64"], _ARGS_VALUES, _ARGS_REQUESTS))
               for form in ("single", "partition")]
# one wider than each limit: (keys, values, requests, the documented error)
OVER_LIMIT = [
    (_WIDE_KEYS, _WIDE_VALUES + [("int64", False)], _WIDE_REQUESTS + [(7, ["sum"])], "Too many distinct value columns"),
    (_WIDE_KEYS + ["int32", "int32"], _WIDE_VALUES, _WIDE_REQUESTS, "Key too wide"),
    (["int64"], _ARGS_VALUES, [(0, ["argmin", "argmax", "sum", "count_all", "sum_of_squares"]), (1, ["argmin", "argmax", "product", "sum"])],
     "Too many distinct accumulators"),
    (["int64"], _ARGS_VALUES + [("int64", False)], [(0, ["argmin", "argmax"]), (1, ["argmin", "argmax"]), (2, ["argmin"])], "Too many ARGMIN"),
]

CASES = _greedy_cases() + LIMIT_CASES


# ------------------------------------------------------------------------------------------------ the ring scatter
class RingCase:
    """Dense integer keys through the ring scatter (paths_dense.cpp try_dense_ring): CUDF_AMD_GB_BIG_MIN_ROWS=1000 opens the path
    to small inputs; enough groups that neither the one-table path T (a table image of at most 96 KiB) nor one hash table takes
    the call; CUDF_AMD_GB_DENSE_LOG2P=11 forces two levels (32-bit tags on the first, then the regions level), which needs a key
    range of more than 2^16 for tables of at least 64 slots - and of more than 2^18 with heavy hitters, whose merged item needs a
    stride of 256 slots."""

    def __init__(self, name, keys, value, kinds, two_level, hot=False):
        self.name = f"ring-{name}-{'two_levels' if two_level else 'one_level'}"
        self.keys, self.value, self.kinds, self.two_level, self.hot = keys, value, kinds, two_level, hot
        self.env = {"CUDF_AMD_GB_BIG_MIN_ROWS": "1000", "CUDF_AMD_GB_ARG_LOOKUP": "0"}
        if two_level:
            self.env["CUDF_AMD_GB_DENSE_LOG2P"] = "11"
        self.n = 200_003 if two_level else 150_001
        self.labels = ring_labels(keys, value, hot, two_level)
        if hot:  # the heavy hitters' partials are merged by the hash-table kernel: partial records of one key unit + NACC units
            self.labels |= {aggregate_records_label("partial", Plan([keys[0][0]], [value], [(0, kinds)]))}

    def __repr__(self):
        return self.name


def build_ring_inputs(case):
    n = case.n
    rng = np.random.default_rng(abs(hash_name(case.name)))
    if len(case.keys) == 1:
        # one key column over a dense range: ~2 rows per key (sizes 1 ... ~10), or with heavy hitters a dozen keys holding a third
        # of the rows
        span = 270_000 if (case.hot and case.two_level) else (90_000 if case.two_level else 40_000)
        k = rng.integers(0, span, n) - 1234
        if case.hot:
            is_hot = rng.random(n) < 1 / 3
            k[is_hot] = rng.integers(0, 12, int(is_hot.sum())) * (span // 13) + 5 - 1234
        cols = [k]
    else:  # two key columns: 700 x 100 values (with the planner's margins a range of ~77,000: more than 2^16)
        cols = [rng.integers(0, 700, n) + (10**12 if case.keys[0][0] == "int64" else -300),
                rng.integers(0, 100, n) - (50 if _cls(case.keys[1][0]) == "i" else 0)]
    keys = []
    for c, (t, nulls) in zip(cols, case.keys):
        keys.append(HostColumn(c.astype(t), (rng.random(n) > 0.1) if nulls else None, t))
    t, nulls = case.value
    data = rng.integers(-50, 51, n)
    data = (data * 0.5).astype(t) if _cls(t) == "f" else data.astype(t)
    valid = None
    if nulls:
        valid = (rng.random(n) > 0.2) & (cols[0] != cols[0][0])  # (one key's values all null)
    return keys, [(HostColumn(data, valid, t), case.kinds)]


_K64, _K32 = ("int64", False), ("int32", False)
RING_CASES = [RingCase(*a, two_level=tl, **kw) for tl in (False, True) for a, kw in (
    (("plain", [_K64], ("int64", False), ["sum", "count_all"]), {}),
    (("heavy_hitters", [_K64], ("float64", False), ["sum", "count_all"]), {"hot": True}),
    (("k32", [_K32], ("int64", False), ["sum", "min", "max"]), {}),
    (("k32_vnull", [_K32], ("float64", True), ["sum", "count_valid", "count_all"]), {}),
    (("k64_vnull", [_K64], ("int64", True), ["sum", "min", "max", "count_valid"]), {}),
    (("k64_k32", [_K64, _K32], ("int64", False), ["sum", "count_all", "max"]), {}),
    (("c4", [_K64, ("int32", True)], ("float64", True), ["mean", "min", "max"]), {}),
    (("run_time_loader", [("int16", False), ("uint8", False)], ("int32", True), ["sum", "count_valid", "count_all", "max"]), {}),
)]

ALL_CASES = CASES + RING_CASES


def predicted_labels():
    return set().union(*(c.labels for c in ALL_CASES))


# Registered instantiations that no input reaches: label -> the dispatch condition that rules it out.
UNREACHABLE = {
}
