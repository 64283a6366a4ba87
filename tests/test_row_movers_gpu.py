"""The partition scatters past their first tile, with sliced columns, checked row for row: cudf::hash_partition (k_hp_scatter) and
cudf::distributed::range_partition / shuffle (k_rp_scatter, fused and one launch per column) at the sizes where a workgroup loops
over a second 4096-row tile and where slices past the 512-workgroup clamp are empty. Every comparison is exact - bitwise for data,
bit for bit for validity - through the row-multiset check of tests/partition_reference.py, which tests/test_partition_reference.py
proves on the CPU. The order of the rows inside a partition is not asserted: the kernels rank rows with LDS atomics.

  2^21          512 slices of exactly one tile: the last size before the tile loop matters
  2^21 + 1      rows per slice round up to 8192: 256 slices of two tiles, one of a single row, 255 empty
  3 * 2^20 + 77 384 slices of two full tiles and one of 77 rows
"""
import functools

import numpy as np
import pytest

import partition_reference as R

pytestmark = pytest.mark.gpu

SIZES = [2**21, 2**21 + 1, 3 * 2**20 + 77]


@pytest.fixture(scope="module")
def G(gpu):
    import gpu_backend
    return gpu_backend


@functools.lru_cache(maxsize=None)
def _table(n):
    """(host columns, device table) of partition_reference.mover_table(n), built and uploaded once per size."""
    import cudf_amd
    import gpu_backend
    cols = R.mover_table(n)
    return cols, cudf_amd.Table([gpu_backend.to_device(c) for c in cols])


def _kernels_of(fn):
    from cudf_amd import _lib
    _lib.profile_reset()
    _lib.profile_enable(True)
    try:
        out = fn()
    finally:
        _lib.profile_enable(False)
    return out, {k: v[0] for k, v in _lib.profile_report().items()}  # {kernel: launches}


def _check_moved(cols, part, out, offs, nparts, what):
    n = len(part)
    assert out.num_rows() == n and out.num_columns() == len(cols)
    assert [int(c.type().id()) for c in out.columns()] == [c.type_id for c in cols], f"{what}: column types"
    assert len(offs) == nparts + 1 and offs[0] == 0 and offs[-1] == n
    assert np.array_equal(np.diff(offs), np.bincount(part, minlength=nparts)), f"{what}: rows per partition"
    for c, o in zip(cols, out.columns()):
        assert o.null_count() == c.null_count, f"{what}: null count"
    R.assert_same_rows(cols, part, [R.raw_host_column(c) for c in out.columns()], offs, what)


# ------------------------------------------------------------------ cudf::hash_partition
@pytest.mark.parametrize("n,nparts", [(n, p) for n in SIZES for p in (3, 64)] + [(2**21 + 1, 4096)])
def test_hash_partition_past_the_slice_clamp(G, oracle, n, nparts):
    """3 partitions take the modulo, 64 the power-of-two mask, 4096 the 139 KiB LDS layout with 16-bit partition ids; the hashed
    int64 and the carried int16 are sliced and nullable."""
    from cudf_amd import partitioning
    cols, t = _table(n)
    (out, offs), kernels = _kernels_of(lambda: partitioning.hash_partition(t, R.HASHED, nparts))
    assert kernels.get("hash_partition_scatter", 0) == 1, kernels
    part, starts, _ = oracle.hash_partition([cols[c] for c in R.HASHED], nparts)
    assert list(offs[:nparts]) == [int(x) for x in starts] and offs[-1] == n
    _check_moved(cols, part, out, offs, nparts, f"hash_partition({n} rows, {nparts} partitions)")


# ------------------------------------------------------------------ cudf::distributed::range_partition
def _destinations(oracle, key_cols, ndest):
    h = oracle.row_hash(key_cols, 0).astype(np.uint64)
    return ((h * np.uint64(ndest)) >> np.uint64(32)).astype(np.int64)


@pytest.mark.parametrize("ndest", [2, 7, 64])
@pytest.mark.parametrize("n", SIZES)
def test_range_partition_past_one_tile(G, oracle, n, ndest):
    """The fused launch (all columns, validity bytes of the two sliced nullable columns included) with 2, 7 and RP_MAX_PARTS = 64
    destinations."""
    from cudf_amd import distributed as D
    cols, t = _table(n)
    (out, offs), kernels = _kernels_of(lambda: D.range_partition(t, R.HASHED, ndest))
    assert kernels.get("range_partition_scatter", 0) == 1, kernels
    dest = _destinations(oracle, [cols[c] for c in R.HASHED], ndest)
    _check_moved(cols, dest, out, offs, ndest, f"range_partition({n} rows, {ndest} destinations)")


def test_range_partition_rejects_65_destinations(G):
    from cudf_amd import distributed as D
    with pytest.raises(ValueError, match="1 to 64 destinations"):
        D.range_partition(_table(SIZES[0])[1], R.HASHED, 65)


@pytest.mark.parametrize("n", SIZES)
def test_range_partition_one_destination_keeps_the_rows(G, n):
    """One destination: the copy branch. Rows in source order, bit for bit (data under a null included: it is a copy), sliced
    columns rebased to row 0."""
    from cudf_amd import distributed as D
    cols, t = _table(n)
    out, offs = D.range_partition(t, R.HASHED, 1)
    assert list(offs) == [0, n] and out.num_rows() == n
    for i, (c, o) in enumerate(zip(cols, out.columns())):
        got = R.raw_host_column(o)
        assert o.offset() == 0 and int(o.type().id()) == c.type_id and o.null_count() == c.null_count
        assert got.data.tobytes() == c.data[c.offset:].tobytes(), f"column {i}: data"
        if c.valid is None:
            assert got.valid is None
        else:
            assert np.array_equal(got.valid, c.valid[c.offset:]), f"column {i}: validity"


# ------------------------------------------------------------------ the pipelined shuffle: one scatter launch per column
def test_shuffle_with_a_peer_past_one_tile(gpu, oracle):
    """World 2 over the loopback transport: rank 0 holds 2^21 + 1 rows, rank 1 five. More than one flat column, so every column is
    scattered by a launch of its own on the side stream - the only way the (c0, c1) form of k_rp_scatter meets a second tile.
    Every received row is owned by its receiver, and the union of the received rows is the union of the sent ones, each rank
    taken as a partition."""
    import cudf_amd
    import gpu_backend
    from cudf_amd import distributed as D
    from loopback_world import run_ranks
    from oracle.oracle import HostColumn
    rng = np.random.default_rng(77)
    world, rows, off = 2, [2**21 + 1, 5], 3
    shards = []
    for n in rows:
        f = rng.integers(-8, 9, n) * 0.5
        f[::5] = -0.0
        f[1::7] = R.NAN_B
        shards.append([HostColumn(rng.integers(-(1 << 40), 1 << 40, n, dtype=np.int64), None, "int64"),
                       HostColumn(f, rng.random(n) > 0.2, "float64"),
                       HostColumn(rng.integers(-(1 << 15), 1 << 15, n + off).astype(np.int16), None, "int16", offset=off)])
    tables = [cudf_amd.Table([gpu_backend.to_device(c) for c in cols]) for cols in shards]

    def rank_fn(r, comm, stream):
        mine = D.shuffle(comm, tables[r], [0], stream=stream)
        return [(R.raw_host_column(c), c.null_count(), int(c.type().id())) for c in mine.columns()]

    res = run_ranks(world, rank_fn)
    received = [res[r][0][0].size for r in range(world)]
    assert sum(received) == sum(rows)
    for r in range(world):
        assert [c[2] for c in res[r]] == [c.type_id for c in shards[0]], f"rank {r}: column types"
        assert np.all(_destinations(oracle, [res[r][0][0]], world) == r), f"rank {r} received a row it does not own"
        for c, (got, nulls, _) in enumerate(res[r]):
            assert got.size == received[r] and nulls == got.null_count, f"rank {r} column {c}: null count"
    sent = [HostColumn(np.concatenate([s[c].data[s[c].offset:] for s in shards]),
                       None if shards[0][c].valid is None else np.concatenate([s[c].valid[s[c].offset:] for s in shards]))
            for c in range(3)]
    got = []
    for c in range(3):
        valid = None
        if any(res[r][c][0].valid is not None for r in range(world)):  # (a rank that received no null has no mask)
            valid = np.concatenate([np.ones(received[r], bool) if res[r][c][0].valid is None else res[r][c][0].valid for r in range(world)])
        got.append(HostColumn(np.concatenate([res[r][c][0].data for r in range(world)]), valid))
    assert sum(res[r][1][1] for r in range(world)) == sum(s[1].null_count for s in shards) > 0
    R.assert_same_rows(sent, _destinations(oracle, [sent[0]], world), got, np.concatenate([[0], np.cumsum(received)]), "shuffle")
