"""GPU tests of cudf::filtered_join (left semi / anti joins) through the C ABI: the golden vectors (tests/golden/kat_semi_anti_join.json),
seeded random inputs against the numpy restatement (tests/filtered_join_restatement.py), each build form and probe forced through the
CUDF_AMD_FJOIN_* settings and proven by the kernels that ran, the all-ones key and a full set at load factor 1, repeated and concurrent probes, the reference's large-extent case, a
100M x 10M property against torch.isin, and the rejected inputs."""
import numpy as np
import pytest

import filtered_join_restatement as R

pytestmark = pytest.mark.gpu

GOLD = R.load_golden()


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


def _check(out, expect):
    assert out.dtype == np.int32
    assert len(out) == len(expect)
    assert np.all(np.diff(out.astype(np.int64)) > 0)  # strictly ascending
    assert out.tolist() == expect.tolist()


def _kernels_of(fn):
    from cudf_amd import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
    finally:
        _lib.profile_enable(False)
    return out, {k: v[0] for k, v in _lib.profile_report().items()}  # {kernel: launches}


def _both(G, left, right, nulls_equal, load_factor=None):
    from cudf_amd.join import FilteredJoin
    from cudf_amd.types import NullEquality
    fj = FilteredJoin(_table(G, right), NullEquality.EQUAL if nulls_equal else NullEquality.UNEQUAL, load_factor=load_factor)
    lt = _table(G, left)
    return _indices(fj.semi_join(lt)), _indices(fj.anti_join(lt))


# ---------------------------------------------------------------- golden vectors
@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: c["name"])
def test_golden(G, c):
    from cudf_amd import join as J
    from cudf_amd.types import NullEquality
    left, right = R.host_table(c["left"]), R.host_table(c["right"])
    eq = c["nulls"] == "equal"
    semi, anti = _both(G, left, right, eq)
    _check(semi, np.array(c["semi"], dtype=np.int32))
    _check(anti, np.array(c["anti"], dtype=np.int32))
    ne = NullEquality.EQUAL if eq else NullEquality.UNEQUAL
    _check(_indices(J.left_semi_join(_table(G, left), _table(G, right), ne)), np.array(c["semi"], dtype=np.int32))
    _check(_indices(J.left_anti_join(_table(G, left), _table(G, right), ne)), np.array(c["anti"], dtype=np.int32))


@pytest.mark.parametrize("path", ["default", "hash_set"])
@pytest.mark.parametrize("c", GOLD["cases"], ids=lambda c: c["name"])
def test_golden_on_each_build_form(G, monkeypatch, c, path):
    """The same vectors with the bitmap ruled out (every key shape on the hash set) and with the bitmap admitted for any range."""
    if path == "hash_set":
        monkeypatch.setenv("CUDF_AMD_FJOIN_DENSE", "0")
    else:
        monkeypatch.setenv("CUDF_AMD_FJOIN_DENSE_RATIO", str(1 << 32))
    semi, anti = _both(G, R.host_table(c["left"]), R.host_table(c["right"]), c["nulls"] == "equal")
    _check(semi, np.array(c["semi"], dtype=np.int32))
    _check(anti, np.array(c["anti"], dtype=np.int32))


@pytest.mark.parametrize("lf", GOLD["invalid_load_factors"]["load_factors"])
def test_invalid_load_factor(G, lf):
    from cudf_amd.join import FilteredJoin
    from cudf_amd.types import NullEquality
    with pytest.raises(ValueError):
        FilteredJoin(_table(G, R.host_table(GOLD["invalid_load_factors"]["right"])), NullEquality.EQUAL, load_factor=lf)


@pytest.mark.parametrize("c", GOLD["rejected_probes"], ids=lambda c: c["name"])
def test_rejected_probes(G, c):
    from cudf_amd.join import FilteredJoin
    fj = FilteredJoin(_table(G, R.host_table(c["right"])))
    err = {"ValueError": ValueError, "TypeError": TypeError}[c["error"]]
    for probe in (fj.semi_join, fj.anti_join):
        with pytest.raises(err):
            probe(_table(G, R.host_table(c["left"])))


@pytest.mark.parametrize("force_set", [False, True])
def test_large_extent(G, monkeypatch, force_set):
    """AntiSemiJoinLargeExtentOverflowPrevention: 10M build rows at load factor 0.004 (about 2.5 G slots when the hash set is
    built); the empty left table of the reference, then a small probe."""
    import torch

    import cudf_amd
    from cudf_amd.join import FilteredJoin
    from cudf_amd.types import NullEquality
    g = GOLD["large_extent"]
    if force_set:
        monkeypatch.setenv("CUDF_AMD_FJOIN_DENSE", "0")
    rk = torch.arange(g["right_sequence_start"], g["right_sequence_start"] + g["right_rows"], dtype=torch.int32, device="cuda")
    fj = FilteredJoin(cudf_amd.Table([cudf_amd.Column.from_torch(rk)]), NullEquality.EQUAL, load_factor=g["load_factor"])
    empty = _table(G, R.host_table(g["left"]))
    assert _indices(fj.semi_join(empty)).tolist() == g["semi"]
    assert _indices(fj.anti_join(empty)).tolist() == g["anti"]
    probe = _table(G, [np.array([5, 10_000_001, -1, 9_999_999, 0, 10_000_000], dtype=np.int32)])
    (semi, anti), k = _kernels_of(lambda: (_indices(fj.semi_join(probe)), _indices(fj.anti_join(probe))))
    assert k.get("fjoin_probe_set" if force_set else "fjoin_probe_bitmap", 0) == 2, k
    assert semi.tolist() == [0, 3, 4] and anti.tolist() == [1, 2, 5]
    del fj
    torch.cuda.synchronize()


# ---------------------------------------------------------------- random inputs against the restatement
TYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool",
         "timestamp_days", "timestamp_ms", "duration_s", "duration_ns", "decimal32", "decimal64"]


def _rand_col(rng, ty, n, universe, null_p, offset=0):
    from oracle.oracle import NP_OF_TYPE_ID, TYPE_ID, HostColumn
    npt = NP_OF_TYPE_ID[TYPE_ID[ty]]
    m = n + offset
    if ty == "bool":
        data = rng.random(m) < 0.5
    elif "float" in ty:
        pool = np.concatenate([[0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf], np.arange(universe) * 0.75 - universe / 3])
        data = pool[rng.integers(0, len(pool), m)].astype(npt)
    else:
        info = np.iinfo(npt)
        lo = max(int(info.min), -(universe // 2)) if info.min < 0 else 0
        data = rng.integers(lo, min(int(info.max), lo + universe - 1), m, endpoint=True).astype(npt)
    valid = rng.random(m) >= null_p if null_p > 0 else None
    return HostColumn(data, valid, ty, offset=offset)


def _compare(G, left, right, nulls_equal, load_factor=None):
    semi, anti = _both(G, left, right, nulls_equal, load_factor)
    es, ea = R.semi_anti(left, right, nulls_equal)
    _check(semi, es)
    _check(anti, ea)
    return semi, anti


@pytest.mark.parametrize("nulls_equal", [True, False])
@pytest.mark.parametrize("ty", TYPES)
def test_random_one_column(G, ty, nulls_equal):
    rng = np.random.default_rng(TYPES.index(ty) * 2 + int(nulls_equal))
    left = [_rand_col(rng, ty, 150_000, 60_000, 0.05, offset=3)]
    right = [_rand_col(rng, ty, 40_000, 60_000, 0.05, offset=7)]
    _compare(G, left, right, nulls_equal)


@pytest.mark.parametrize("nulls_equal", [True, False])
@pytest.mark.parametrize("types", [("int32", "int32"), ("int64", "float64"), ("int8", "uint16", "float32"), ("bool", "int64", "decimal32")],
                         ids=lambda t: "_".join(t))
def test_random_several_columns(G, types, nulls_equal):
    rng = np.random.default_rng(len(types) * 10 + int(nulls_equal) + sum(map(len, types)))
    left = [_rand_col(rng, ty, 120_000, 12, 0.04, offset=i) for i, ty in enumerate(types)]
    right = [_rand_col(rng, ty, 30_000, 12, 0.04, offset=2 * i) for i, ty in enumerate(types)]
    _compare(G, left, right, nulls_equal)


@pytest.mark.parametrize("shape", ["heavy_duplicates", "all_hit", "no_hit", "all_null_build"])
@pytest.mark.parametrize("ty", ["int32", "int64", "float64"])
def test_random_shapes(G, shape, ty):
    from oracle.oracle import HostColumn
    rng = np.random.default_rng(["heavy_duplicates", "all_hit", "no_hit", "all_null_build"].index(shape) + 100)
    npt = {"int32": np.int32, "int64": np.int64, "float64": np.float64}[ty]
    if shape == "heavy_duplicates":  # 400,000 build rows over 50 keys
        right = [HostColumn(rng.integers(0, 50, 400_000).astype(npt))]
        left = [HostColumn(rng.integers(0, 100, 300_000).astype(npt), rng.random(300_000) > 0.1)]
    elif shape == "all_hit":
        right = [HostColumn(np.arange(70_000).astype(npt))]
        left = [HostColumn(rng.integers(0, 70_000, 500_000).astype(npt))]
    elif shape == "no_hit":
        right = [HostColumn(np.arange(70_000).astype(npt))]
        left = [HostColumn(rng.integers(70_000, 900_000, 500_000).astype(npt))]
    else:
        right = [HostColumn(np.arange(1000).astype(npt), np.zeros(1000, dtype=bool))]
        left = [HostColumn(rng.integers(0, 1000, 10_000).astype(npt), rng.random(10_000) > 0.5)]
    for eq in (True, False):
        semi, anti = _compare(G, left, right, eq)
    if shape == "all_hit":
        assert len(anti) == 0
    if shape == "no_hit":
        assert len(semi) == 0


# ---------------------------------------------------------------- each path, forced and proven
@pytest.mark.parametrize("kind", ["semi", "anti"])
@pytest.mark.parametrize("path", ["lds_bitmap", "global_bitmap", "hash_set"])
@pytest.mark.parametrize("ty", ["int16", "int32", "uint64"])
def test_each_path(G, monkeypatch, ty, path, kind):
    from cudf_amd.join import FilteredJoin
    from cudf_amd.types import NullEquality
    if path == "global_bitmap":
        monkeypatch.setenv("CUDF_AMD_FJOIN_LDS_BITS", "0")
    if path == "hash_set":
        monkeypatch.setenv("CUDF_AMD_FJOIN_DENSE", "0")
    rng = np.random.default_rng(["lds_bitmap", "global_bitmap", "hash_set"].index(path) * 7 + len(ty))
    left = [_rand_col(rng, ty, 400_000, 30_000, 0.05, offset=5)]
    right = [_rand_col(rng, ty, 20_000, 20_000, 0.05, offset=1)]
    for eq in (True, False):
        fj = FilteredJoin(_table(G, right), NullEquality.EQUAL if eq else NullEquality.UNEQUAL)
        lt = _table(G, left)
        out, k = _kernels_of(lambda: _indices(getattr(fj, kind + "_join")(lt)))
        expect = R.semi_anti(left, right, eq)[kind == "anti"]
        _check(out, expect)
        probe = {"lds_bitmap": "fjoin_probe_lds", "global_bitmap": "fjoin_probe_bitmap", "hash_set": "fjoin_probe_set"}[path]
        assert k.get(probe, 0) == 1 and k.get("fjoin_compact", 0) == 1, k
        others = {"fjoin_probe_lds", "fjoin_probe_bitmap", "fjoin_probe_set"} - {probe}
        assert not any(k.get(o, 0) for o in others), k


def test_bitmap_admission(G, monkeypatch):
    """A 4-byte key column whose build range exceeds CUDF_AMD_FJOIN_DENSE_RATIO bits per build row takes the hash set; within it,
    the bitmap."""
    from oracle.oracle import HostColumn
    right = [HostColumn(np.array([0, 1000, 5000], dtype=np.int32))]
    left = [HostColumn(np.array([5000, 7, 1000, 0], dtype=np.int32))]
    for ratio, built in ((1 << 20, "fjoin_bitmap_build"), (8, "fjoin_set_build")):
        monkeypatch.setenv("CUDF_AMD_FJOIN_DENSE_RATIO", str(ratio))
        (semi, anti), k = _kernels_of(lambda: _both(G, left, right, True))
        assert k.get(built, 0) == 1, k
        assert semi.tolist() == [0, 2, 3] and anti.tolist() == [1]


# ---------------------------------------------------------------- the slot walk at its edges
@pytest.mark.parametrize("present", [True, False], ids=["present", "absent"])
@pytest.mark.parametrize("ty", ["int64", "uint64"])
def test_all_ones_key_on_the_hash_set(G, monkeypatch, ty, present):
    """The 8-byte key whose bits are all ones (int64 -1, uint64 2^64 - 1) is the word of an empty slot: the inline set keeps it in a
    flag instead. 1,000 rows a side with duplicates and a few NULLs; the key on both sides, or on the probe side only."""
    from oracle.oracle import HostColumn
    from cudf_amd.join import FilteredJoin
    from cudf_amd.types import NullEquality
    monkeypatch.setenv("CUDF_AMD_FJOIN_DENSE", "0")
    rng = np.random.default_rng(["int64", "uint64"].index(ty) * 2 + int(present))
    npt = np.dtype(ty).type
    ones = npt(-1) if ty == "int64" else npt(2**64 - 1)
    rdata, ldata = rng.integers(0, 600, 1000).astype(npt), rng.integers(0, 1200, 1000).astype(npt)
    if present:
        rdata[[3, 500, 999]] = ones
    ldata[[0, 17, 64, 511, 999]] = ones
    lvalid = rng.random(1000) >= 0.01
    lvalid[0] = True
    right = [HostColumn(rdata, rng.random(1000) >= 0.01, ty)]
    left = [HostColumn(ldata, lvalid, ty)]
    lt = _table(G, left)
    for eq in (True, False):
        fj, k = _kernels_of(lambda: FilteredJoin(_table(G, right), NullEquality.EQUAL if eq else NullEquality.UNEQUAL))
        assert k.get("fjoin_set_build", 0) == 1 and not k.get("fjoin_bitmap_build"), k
        expect = R.semi_anti(left, right, eq)
        assert (0 in expect[0].tolist()) == present  # (left row 0 holds the key)
        for kind in ("semi", "anti"):
            out, k = _kernels_of(lambda: _indices(getattr(fj, kind + "_join")(lt)))
            _check(out, expect[kind == "anti"])
            assert k.get("fjoin_probe_set", 0) == 1 and k.get("fjoin_compact", 0) == 1, k


@pytest.mark.parametrize("form", ["inline", "rows"])
def test_full_set_wraps_and_ends_at_its_one_empty_slot(G, monkeypatch, form):
    """Load factor 1.0: 257 distinct build keys in 258 slots (rows + 1). The walks run through long clusters, wrap at the last slot,
    and every absent key ends at the single empty slot. 4,096 probe keys, half of them absent; the inline set (one int64 column)
    and {hash | row} slots (two columns)."""
    from oracle.oracle import HostColumn
    monkeypatch.setenv("CUDF_AMD_FJOIN_DENSE", "0")
    rng = np.random.default_rng(258 + len(form))
    pool = rng.choice(1 << 40, 257 + 2048, replace=False).astype(np.int64)
    build, absent = pool[:257], pool[257:]
    probe = rng.permutation(np.concatenate([build[rng.integers(0, 257, 2048)], absent]))
    right, left = [HostColumn(build)], [HostColumn(probe)]
    if form == "rows":
        right.append(HostColumn(build ^ 0x5555))
        left.append(HostColumn(probe ^ 0x5555))
    (semi, anti), k = _kernels_of(lambda: _compare(G, left, right, False, load_factor=1.0))
    assert len(semi) == 2048 and len(anti) == 2048
    assert k.get("fjoin_set_build", 0) == 1 and k.get("fjoin_probe_set", 0) == 2 and k.get("fjoin_compact", 0) == 2, k


# ---------------------------------------------------------------- one object, many probes, two streams
def test_repeated_and_concurrent_probes(G, monkeypatch):
    import torch

    from cudf_amd.join import FilteredJoin
    from cudf_amd.types import NullEquality
    rng = np.random.default_rng(5)
    right = [_rand_col(rng, "int64", 100_000, 300_000, 0.05)]
    lefts = [[_rand_col(rng, "int64", 250_000, 400_000, 0.05, offset=i)] for i in range(4)]
    for dense in ("1", "0"):  # the bitmap, then the hash set
        monkeypatch.setenv("CUDF_AMD_FJOIN_DENSE", dense)
        fj = FilteredJoin(_table(G, right), NullEquality.UNEQUAL)
        expects = [R.semi_anti(l, right, False) for l in lefts]
        tables = [_table(G, l) for l in lefts]
        for _ in range(2):  # the same object, probed again
            for t, (es, ea) in zip(tables, expects):
                _check(_indices(fj.semi_join(t)), es)
                _check(_indices(fj.anti_join(t)), ea)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        for i, t in enumerate(tables):
            st = s1 if i % 2 == 0 else s2
            outs.append((fj.semi_join(t, stream=st), fj.anti_join(t, stream=st)))
        s1.synchronize()
        s2.synchronize()
        for (semi, anti), (es, ea) in zip(outs, expects):
            _check(_indices(semi), es)
            _check(_indices(anti), ea)
        del fj


# ---------------------------------------------------------------- property at scale
@pytest.mark.parametrize("keys", ["dense", "sparse"])
def test_property_100m_probe_10m_build(G, keys):
    """100M probe rows x 10M build rows, 5 % nulls on both sides, UNEQUAL: the semi count is the number of valid probe keys
    torch.isin finds among the valid build keys, semi + anti is every row, both ascending."""
    import torch

    import cudf_amd
    from bench_configs import bernoulli_mask
    from cudf_amd.join import FilteredJoin
    from cudf_amd.types import NullEquality
    dev = torch.device("cuda", 0)
    nl, nr = 100_000_000, 10_000_000
    g = torch.Generator(device=dev).manual_seed(77)
    rk = torch.randint(0, 2 * nr, (nr,), generator=g, device=dev, dtype=torch.int64)
    lk = torch.randint(0, 3 * nr, (nl,), generator=g, device=dev, dtype=torch.int64)
    if keys == "sparse":
        rk, lk = rk * 1_000_003, lk * 1_000_003
    lm, lnulls, lvalid = bernoulli_mask(nl, 0.05, 1, dev)
    rm, rnulls, rvalid = bernoulli_mask(nr, 0.05, 2, dev)
    expect = int((torch.isin(lk, rk[rvalid]) & lvalid).sum())
    fj = FilteredJoin(cudf_amd.Table([cudf_amd.Column.from_torch(rk, rm, rnulls)]), NullEquality.UNEQUAL)
    L = cudf_amd.Table([cudf_amd.Column.from_torch(lk, lm, lnulls)])
    (semi, anti), k = _kernels_of(lambda: (fj.semi_join(L), fj.anti_join(L)))
    assert k.get("fjoin_probe_bitmap" if keys == "dense" else "fjoin_probe_set", 0) == 2, k
    s, a = semi.to_torch().long(), anti.to_torch().long()
    assert s.numel() == expect and s.numel() + a.numel() == nl
    assert bool((s[1:] > s[:-1]).all()) and bool((a[1:] > a[:-1]).all())
    hit = torch.zeros(nl, dtype=torch.bool, device=dev)
    hit[s] = True
    assert not bool(hit[a].any())
    del fj
    torch.cuda.synchronize()
