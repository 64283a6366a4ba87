"""GPU tests of cudf::distinct_hash_join through the C ABI: the golden vectors (tests/golden/kat_distinct_join.json), seeded random
inputs with a distinct build side against the numpy restatement (tests/distinct_join_restatement.py, compared exactly), each build
form forced through CUDF_AMD_DJOIN_DENSE and proven by the kernels that ran, the boundaries of the probe's chunk geometry, load
factor 1, the key equal to the empty-slot value, null build rows, duplicate build rows (harmless), repeated and concurrent probes,
the reference's large-extent case, a 20M x 2M property against torch.isin, and the rejected inputs."""
import numpy as np
import pytest

import distinct_join_restatement as R
import filtered_join_restatement as FR
from test_filtered_join_gpu import TYPES, _rand_col

pytestmark = pytest.mark.gpu

GOLD = R.load_golden()
NM = R.JoinNoMatch
FORMS = ["direct", "map"]
KERNELS = {"djoin_build_direct", "djoin_build_map", "djoin_probe_direct", "djoin_probe_map", "djoin_compact"}


@pytest.fixture(scope="module")
def G(gpu):
    import gpu_backend
    return gpu_backend


def _table(G, cols):
    import cudf_amd
    return cudf_amd.Table([G.to_device(c) for c in cols])


def _indices(col):
    assert col.type().id().name == "INT32" and col.null_count() == 0
    return col.to_numpy()[0]


def _kernels_of(fn):
    from cudf_amd import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
    finally:
        _lib.profile_enable(False)
    return out, {k: v[0] for k, v in _lib.profile_report().items() if k in KERNELS and v[0] > 0}  # {kernel: launches}


def _force(monkeypatch, form):
    """direct: the default admission; map: the direct table ruled out."""
    monkeypatch.setenv("CUDF_AMD_DJOIN_DENSE", "0" if form == "map" else "1")


def _object(G, right, nulls_equal, load_factor=None):
    from cudf_amd.join import DistinctHashJoin
    from cudf_amd.types import NullEquality
    return DistinctHashJoin(_table(G, right), NullEquality.EQUAL if nulls_equal else NullEquality.UNEQUAL, load_factor=load_factor)


def _probe_both(dj, lt, nl):
    """(left_join, inner left, inner right) of one probe table, with the contract's shape checks."""
    lj = _indices(dj.left_join(lt))
    li, ri = map(_indices, dj.inner_join(lt))
    assert lj.dtype == np.int32 and len(lj) == nl
    assert len(li) == len(ri)
    assert np.all(np.diff(li.astype(np.int64)) > 0)  # strictly ascending
    return lj, li, ri


def _compare(G, left, right, nulls_equal, load_factor=None, dj=None):
    """Both joins of (left, right) equal the restatement exactly (the build side is distinct)."""
    dj = dj or _object(G, right, nulls_equal, load_factor)
    nl = left[0].size if left else 0
    lj, li, ri = _probe_both(dj, _table(G, left), nl)
    expect = R.right_of_left(left, right, nulls_equal)
    hit = expect != NM
    assert np.array_equal(lj, expect)
    assert np.array_equal(li, np.flatnonzero(hit).astype(np.int32)) and np.array_equal(ri, expect[hit])
    return lj


def _with_offset(c, k):
    """The same rows behind k leading elements of the buffers (a sliced column)."""
    from oracle.oracle import HostColumn
    data = np.asarray(c.data)[c.offset:c.offset + c.size]
    valid = None if c.valid is None else np.asarray(c.valid[c.offset:c.offset + c.size], dtype=bool)
    data = np.concatenate([data[:1].repeat(k), data])
    valid = None if valid is None else np.concatenate([np.ones(k, dtype=bool), valid])
    return HostColumn(data, valid, R._NAME_OF_TYPE_ID[c.type_id], offset=k)


def _col(data, valid=None):
    from oracle.oracle import HostColumn
    return HostColumn(np.asarray(data), None if valid is None else np.asarray(valid, dtype=bool))


# ---------------------------------------------------------------- golden vectors
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: c["name"])
def test_golden(G, monkeypatch, c, form):
    _force(monkeypatch, form)
    left, right = R.case_tables(c)
    expect = R.case_expected(c)
    nl = left[0].size
    for lf in c["load_factors"]:
        dj = _object(G, right, c["nulls"] == "equal", lf)
        lj, li, ri = _probe_both(dj, _table(G, left), nl)
        if "inner" in expect:
            assert li.tolist() == expect["inner"][0].tolist() and ri.tolist() == expect["inner"][1].tolist()
        if "left_join" in expect:
            assert lj.tolist() == expect["left_join"].tolist()
        _compare(G, left, right, c["nulls"] == "equal", dj=dj)


@pytest.mark.parametrize("lf", GOLD["invalid_load_factors"]["load_factors"])
def test_invalid_load_factor(G, lf):
    with pytest.raises(ValueError):
        _object(G, R.host_table(GOLD["invalid_load_factors"]["right"]), True, lf)


def test_right_table_without_columns(G):
    from cudf_amd._lib import CudfAmdError
    with pytest.raises(CudfAmdError):
        _object(G, [], True)


@pytest.mark.parametrize("c", FR.load_golden()["rejected_probes"], ids=lambda c: c["name"])
def test_rejected_probes(G, c):
    dj = _object(G, R.host_table(c["right"]), True)
    err = {"ValueError": ValueError, "TypeError": TypeError}[c["error"]]
    for probe in (dj.inner_join, dj.left_join):
        with pytest.raises(err):
            probe(_table(G, R.host_table(c["left"])))


@pytest.mark.parametrize("form", FORMS)
def test_large_extent(G, monkeypatch, form):
    """DistinctLargeExtentOverflowPrevention: 10M build rows at load factor 0.004 (about 2.5 G slots when the map is built); the
    empty left table of the reference, then a small probe."""
    import torch

    import cudf_amd
    from cudf_amd.join import DistinctHashJoin
    from cudf_amd.types import NullEquality
    g = GOLD["large_extent"]
    _force(monkeypatch, form)
    n = g["right_rows"]
    rk = torch.arange(g["right_sequence_start"], g["right_sequence_start"] + n, dtype=torch.int32, device="cuda")
    dj = DistinctHashJoin(cudf_amd.Table([cudf_amd.Column.from_torch(rk)]), NullEquality.EQUAL, load_factor=g["load_factor"])
    empty = _table(G, R.host_table(g["left"]))
    li, ri = map(_indices, dj.inner_join(empty))
    assert li.tolist() == g["inner"]["left"] and ri.tolist() == g["inner"]["right"]
    assert _indices(dj.left_join(empty)).tolist() == []
    probe = _table(G, [np.array([0, n - 1, -1, n, n + 1, 5], dtype=np.int32)])
    (lj, li, ri), k = _kernels_of(lambda: _probe_both(dj, probe, 6))
    assert k == {"djoin_probe_" + form: 2, "djoin_compact": 1}, k
    assert lj.tolist() == [0, n - 1, NM, NM, NM, 5]
    assert li.tolist() == [0, 1, 5] and ri.tolist() == [0, n - 1, 5]
    del dj
    torch.cuda.synchronize()


# ---------------------------------------------------------------- random inputs against the restatement
@pytest.mark.parametrize("nulls_equal", [True, False])
@pytest.mark.parametrize("ty", TYPES)
def test_random_one_column(G, ty, nulls_equal):
    rng = np.random.default_rng(TYPES.index(ty) * 2 + int(nulls_equal))
    left = [_rand_col(rng, ty, 150_000, 60_000, 0.05, offset=3)]
    right = [_with_offset(c, 7) for c in R.distinct_rows([_rand_col(rng, ty, 40_000, 60_000, 0.05)])]
    assert 1 < right[0].size <= 40_000
    lj = _compare(G, left, right, nulls_equal)
    assert (lj != NM).any()


@pytest.mark.parametrize("nulls_equal", [True, False])
@pytest.mark.parametrize("types", [("int32", "int32"), ("int64", "float64"), ("int8", "uint16", "float32"), ("bool", "int64", "decimal32")],
                         ids=lambda t: "_".join(t))
def test_random_several_columns(G, types, nulls_equal):
    rng = np.random.default_rng(len(types) * 10 + int(nulls_equal) + sum(map(len, types)))
    left = [_rand_col(rng, ty, 120_000, 12, 0.04, offset=i) for i, ty in enumerate(types)]
    right = R.distinct_rows([_rand_col(rng, ty, 30_000, 12, 0.04) for ty in types])
    right = [_with_offset(c, 2 * i + 1) for i, c in enumerate(right)]
    lj = _compare(G, left, right, nulls_equal)
    assert (lj != NM).any()


# ---------------------------------------------------------------- boundaries of the probe's geometry
@pytest.mark.parametrize("shape", ["all_hit", "no_hit", "out_of_range"])
@pytest.mark.parametrize("form", FORMS)
def test_boundaries(G, monkeypatch, form, shape):
    """Left row counts around the ballot word (64), the 8 x 64-row step (512) and the chunk and wave-count edges of geometry_of
    (65,537 rows: 17 chunks in 32 waves), on a 1,000-row build of the even keys of [0, 2000)."""
    _force(monkeypatch, form)
    rng = np.random.default_rng(FORMS.index(form) * 3 + len(shape))
    right = [_col((rng.permutation(1000) * 2).astype(np.int32))]
    (dj, _), k = _kernels_of(lambda: (_object(G, right, True), None))
    assert k == {"djoin_build_" + form: 1}, k
    for n in (1, 63, 64, 65, 511, 512, 513, 65_537):
        if shape == "all_hit":
            keys = rng.integers(0, 1000, n) * 2
        elif shape == "no_hit":  # inside the direct table's range
            keys = rng.integers(0, 999, n) * 2 + 1
        else:
            keys = np.where(rng.random(n) < 0.5, rng.integers(2000, 1 << 30, n), -rng.integers(1, 1 << 30, n))
        lj = _compare(G, [_col(keys.astype(np.int32))], right, True, dj=dj)
        assert bool((lj != NM).all()) if shape == "all_hit" else bool((lj == NM).all())


@pytest.mark.parametrize("key", ["int32", "int64", "two_columns"])
def test_load_factor_one_all_misses(G, monkeypatch, key):
    """The map holds at least rows + 1 slots: at load factor 1.0 a probe of keys that are all absent ends (at the one empty slot)."""
    _force(monkeypatch, "map")
    rng = np.random.default_rng(11)
    npt = np.int32 if key == "int32" else np.int64
    build = rng.permutation(4000)[:2000].astype(npt)
    right = [_col(build)] + ([_col(np.arange(2000, dtype=np.int32))] if key == "two_columns" else [])
    miss = rng.integers(5000, 1 << 30, 20_000).astype(npt)
    left = [_col(miss)] + ([_col(rng.integers(0, 2000, 20_000).astype(np.int32))] if key == "two_columns" else [])
    (dj, _), k = _kernels_of(lambda: (_object(G, right, True, 1.0), None))
    assert k == {"djoin_build_map": 1}, k
    assert bool((_compare(G, left, right, True, dj=dj) == NM).all())
    assert _compare(G, right, right, True, dj=dj).tolist() == list(range(2000))  # and every build row finds itself


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("present", [True, False])
@pytest.mark.parametrize("ty", ["int64", "uint64"])
def test_key_equal_to_the_empty_slot_value(G, monkeypatch, ty, present, form):
    """The 8-byte key whose bits are all ones (int64 -1, uint64 2^64 - 1) cannot live in a slot: it has a side word."""
    _force(monkeypatch, form)
    ones = -1 if ty == "int64" else 2**64 - 1
    right = [_col(np.array([5, ones if present else 6, 7, 3], dtype=ty))]
    left = [_col(np.array([ones, 5, 9, ones, 3], dtype=ty), [True, True, True, False, True])]
    for eq in (True, False):
        lj = _compare(G, left, right, eq)
        assert lj.tolist() == [1 if present else NM, 0, NM, NM, 3]


@pytest.mark.parametrize("layout", ["direct_int32", "direct_int8", "key4_int32", "key4_float32", "key8_int64", "key8_float64"])
def test_null_build_row(G, monkeypatch, layout):
    """nulls EQUAL: a NULL probe key answers THE ROW of the NULL build key, in each single-column layout; UNEQUAL: nothing."""
    form, ty = layout.split("_")
    _force(monkeypatch, "direct" if form == "direct" else "map")
    right = [_col(np.array([10, 99, 30], dtype=ty), [True, False, True])]
    left = [_col(np.array([0, 30, 99, 0, 10], dtype=ty), [False, True, True, False, True])]
    (lj, k) = _kernels_of(lambda: _compare(G, left, right, True))
    assert k.get("djoin_build_" + ("direct" if form == "direct" else "map"), 0) == 1, k
    assert lj.tolist() == [1, 2, NM, 1, 0]
    assert _compare(G, left, right, False).tolist() == [NM, 2, NM, NM, 0]
    # no NULL build key: a NULL probe key matches nothing under either setting
    right = [_col(np.array([10, 99, 30], dtype=ty))]
    assert _compare(G, left, right, True).tolist() == [NM, 2, 1, NM, 0]


# ---------------------------------------------------------------- each path, forced and proven
@pytest.mark.parametrize("op", ["left_join", "inner_join"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("key", ["int16", "int32", "uint64", "two_columns"])
def test_each_path(G, monkeypatch, key, form, op):
    _force(monkeypatch, form)
    ran = "map" if key == "two_columns" else form  # (only one integer column can take the direct table)
    rng = np.random.default_rng(FORMS.index(form) * 7 + len(key))
    types = ["int32", "int64"] if key == "two_columns" else [key]
    universe = 300 if key == "two_columns" else 30_000
    left = [_rand_col(rng, ty, 400_000, universe, 0.05, offset=5) for ty in types]
    right = [_with_offset(c, 1) for c in R.distinct_rows([_rand_col(rng, ty, 20_000, universe, 0.05) for ty in types])]
    lt = _table(G, left)
    for eq in (True, False):
        expect = R.right_of_left(left, right, eq)
        hit = expect != NM
        dj, k = _kernels_of(lambda: _object(G, right, eq))
        assert k == {"djoin_build_" + ran: 1}, k
        if op == "left_join":
            out, k = _kernels_of(lambda: _indices(dj.left_join(lt)))
            assert np.array_equal(out, expect)
            assert k == {"djoin_probe_" + ran: 1}, k
        else:
            (li, ri), k = _kernels_of(lambda: tuple(map(_indices, dj.inner_join(lt))))
            assert np.array_equal(li, np.flatnonzero(hit).astype(np.int32)) and np.array_equal(ri, expect[hit])
            assert k == {"djoin_probe_" + ran: 1, "djoin_compact": 1}, k


def test_direct_admission(G, monkeypatch):
    """A 4-byte key column whose build range exceeds CUDF_AMD_DJOIN_DENSE_RATIO entries per build row, or
    CUDF_AMD_DJOIN_DENSE_MAX_BYTES, takes the map; within both, the direct table."""
    right = [_col(np.array([0, 1000, 5000], dtype=np.int32))]
    left = [_col(np.array([5000, 7, 1000, 0, -3], dtype=np.int32))]
    for ratio, max_bytes, built in ((1 << 20, 1 << 31, "direct"), (8, 1 << 31, "map"), (1 << 20, 4 * 5000, "map"), (1 << 20, 4 * 5001, "direct")):
        monkeypatch.setenv("CUDF_AMD_DJOIN_DENSE_RATIO", str(ratio))
        monkeypatch.setenv("CUDF_AMD_DJOIN_DENSE_MAX_BYTES", str(max_bytes))
        lj, k = _kernels_of(lambda: _compare(G, left, right, True))
        assert k.get("djoin_build_" + built, 0) == 1 and k.get("djoin_probe_" + built, 0) == 2, k
        assert lj.tolist() == [2, NM, 1, 0, NM]


# ---------------------------------------------------------------- duplicate build rows are harmless
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("ty", ["int32", "int64"])
def test_duplicate_build_rows(G, monkeypatch, ty, form):
    """400,000 build rows over 50 keys: the calls return, every left row gets ONE of its equal build rows, and the matched left rows
    are filtered_join's semi join."""
    _force(monkeypatch, form)
    rng = np.random.default_rng(21)
    rk = rng.integers(0, 50, 400_000).astype(ty)
    lk = rng.integers(0, 100, 300_000).astype(ty)
    lvalid = rng.random(300_000) > 0.1
    left, right = [_col(lk, lvalid)], [_col(rk)]
    lt = _table(G, left)
    for eq in (True, False):
        dj = _object(G, right, eq)
        lj, li, ri = _probe_both(dj, lt, 300_000)
        semi = FR.semi_anti(left, right, eq)[0]
        assert np.array_equal(np.flatnonzero(lj != NM).astype(np.int32), semi) and np.array_equal(li, semi)
        assert np.array_equal(ri, lj[semi])
        assert ri.min() >= 0 and ri.max() < 400_000
        assert np.array_equal(rk[ri], lk[li]) and bool(lvalid[li].all())
        lj2, _, _ = _probe_both(dj, lt, 300_000)  # one object names the same row every time
        assert np.array_equal(lj, lj2)


# ---------------------------------------------------------------- one object, many probes, two streams
def test_repeated_and_concurrent_probes(G, monkeypatch):
    import torch
    rng = np.random.default_rng(5)
    right = R.distinct_rows([_rand_col(rng, "int64", 100_000, 300_000, 0.05)])
    lefts = [[_rand_col(rng, "int64", 250_000, 400_000, 0.05, offset=i)] for i in range(4)]
    expects = [R.right_of_left(l, right, False) for l in lefts]
    for form in FORMS:
        _force(monkeypatch, form)
        dj, k = _kernels_of(lambda: _object(G, right, False))
        assert k == {"djoin_build_" + form: 1}, k
        tables = [_table(G, l) for l in lefts]

        def check(lj, li, ri, e):
            hit = e != NM
            assert np.array_equal(lj, e) and np.array_equal(li, np.flatnonzero(hit).astype(np.int32)) and np.array_equal(ri, e[hit])

        for _ in range(2):  # the same object, probed again
            for t, e in zip(tables, expects):
                check(*_probe_both(dj, t, 250_000), e)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        for i, t in enumerate(tables):
            st = s1 if i % 2 == 0 else s2
            outs.append((dj.left_join(t, stream=st), dj.inner_join(t, stream=st)))
        s1.synchronize()
        s2.synchronize()
        for (lj, (li, ri)), e in zip(outs, expects):
            check(_indices(lj), _indices(li), _indices(ri), e)
        del dj


# ---------------------------------------------------------------- property at scale
@pytest.mark.parametrize("keys", ["dense", "sparse"])
def test_property_20m_probe_2m_build(G, keys):
    """20M probe rows x 2M distinct build keys made on the device, 5 % nulls on both sides, UNEQUAL: the inner_join count is the number
    of valid probe keys torch.isin finds among the valid build keys, the keys at the returned pairs are equal, and left_join's
    matches are the inner right indices in order."""
    import torch

    import cudf_amd
    from bench_configs import bernoulli_mask
    from cudf_amd.join import DistinctHashJoin
    from cudf_amd.types import NullEquality
    dev = torch.device("cuda", 0)
    nl, nr = 20_000_000, 2_000_000
    g = torch.Generator(device=dev).manual_seed(78)
    rk = torch.randperm(2 * nr, generator=g, device=dev)[:nr].to(torch.int64).contiguous()
    lk = torch.randint(0, 3 * nr, (nl,), generator=g, device=dev, dtype=torch.int64)
    if keys == "sparse":
        rk, lk = rk * 1_000_003, lk * 1_000_003
    lm, lnulls, lvalid = bernoulli_mask(nl, 0.05, 1, dev)
    rm, rnulls, rvalid = bernoulli_mask(nr, 0.05, 2, dev)
    expect = int((torch.isin(lk, rk[rvalid]) & lvalid).sum())
    form = "direct" if keys == "dense" else "map"
    dj, k = _kernels_of(lambda: DistinctHashJoin(cudf_amd.Table([cudf_amd.Column.from_torch(rk, rm, rnulls)]), NullEquality.UNEQUAL))
    assert k == {"djoin_build_" + form: 1}, k
    L = cudf_amd.Table([cudf_amd.Column.from_torch(lk, lm, lnulls)])
    (lj, (li, ri)), k = _kernels_of(lambda: (dj.left_join(L), dj.inner_join(L)))
    assert k == {"djoin_probe_" + form: 2, "djoin_compact": 1}, k
    lj, li, ri = lj.to_torch(), li.to_torch().long(), ri.to_torch()
    assert lj.numel() == nl and li.numel() == expect and ri.numel() == expect
    assert bool((li[1:] > li[:-1]).all())
    assert bool((lk[li] == rk[ri.long()]).all()) and bool(lvalid[li].all()) and bool(rvalid[ri.long()].all())
    hit = lj != NM
    assert bool((torch.nonzero(hit).flatten() == li).all()) and bool((lj[hit] == ri).all())
    del dj
    torch.cuda.synchronize()
