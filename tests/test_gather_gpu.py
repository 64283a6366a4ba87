"""cudf::gather at its block, wave and word edges, against np.take on the host, exactly (bitwise data where valid, validity bit for
bit, null counts). Nine source columns, so k_gather_multi is launched three times (4 + 4 + 1 columns) with stores of 1, 2, 4 and
8 bytes; 70,001 source rows, a multiple of nothing; map lengths either side of 32 (k_gather_mask writes one word per half wave),
64 (one wave), 256 (one block of k_gather_mask, one stride of k_gather_multi) and 1024 (one block of k_gather_multi: four strides of
256). Sliced source columns, a sliced map, a source of no rows and a map of no rows."""
import numpy as np
import pytest

import partition_reference as R

pytestmark = pytest.mark.gpu

SRC_ROWS = 70_001
LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1


def _source(n, seed=5):
    """int8, uint16 nullable, int32 sliced at 3, int64 nullable sliced at 37, float32, float64 nullable without a null, bool,
    uint8, int16."""
    from oracle.oracle import HostColumn
    rng = np.random.default_rng(seed)
    f32 = (rng.integers(-4, 5, n) * 0.5).astype(np.float32)
    f32[::9] = -0.0
    f32[4::11] = np.array([0x7fc00123], np.uint32).view(np.float32)[0]
    f64 = rng.integers(-4, 5, n) * 0.25
    f64[::7] = -0.0
    f64[3::13] = R.NAN_B
    return [
        HostColumn(rng.integers(-128, 128, n).astype(np.int8), None, "int8"),
        HostColumn(rng.integers(0, 1 << 16, n).astype(np.uint16), rng.random(n) > 0.25, "uint16"),
        HostColumn(rng.integers(-(1 << 31), 1 << 31, n + 3).astype(np.int32), None, "int32", offset=3),
        HostColumn(rng.integers(-(1 << 62), 1 << 62, n + 37, dtype=np.int64), rng.random(n + 37) > 0.4, "int64", offset=37),
        HostColumn(f32, None, "float32"),
        HostColumn(f64, np.ones(n, bool), "float64"),
        HostColumn(rng.integers(0, 3, n).astype(np.uint8), None, "bool"),
        HostColumn(rng.integers(0, 256, n).astype(np.uint8), None, "uint8"),
        HostColumn(rng.integers(-(1 << 15), 1 << 15, n).astype(np.int16), None, "int16"),
    ]


@pytest.fixture(scope="module")
def source(gpu):
    import cudf_amd
    import gpu_backend
    cols = _source(SRC_ROWS)
    return cols, cudf_amd.Table([gpu_backend.to_device(c) for c in cols])


@pytest.fixture(scope="module")
def empty_source(gpu):
    import cudf_amd
    import gpu_backend
    cols = _source(0)
    return cols, cudf_amd.Table([gpu_backend.to_device(c) for c in cols])


def _gather(table, idx, policy, offset=0):
    """idx[offset:] is the map: with an offset the map column is a slice of the uploaded buffer."""
    import cudf_amd
    from cudf_amd import partitioning
    from cudf_amd.types import OutOfBoundsPolicy
    gmap = cudf_amd.Column.from_numpy(np.asarray(idx, np.int32), offset=offset)
    return partitioning.gather(table, gmap, OutOfBoundsPolicy.NULLIFY if policy == "nullify" else OutOfBoundsPolicy.DONT_CHECK)


def _check(cols, out, idx, nullify):
    """np.take of every source column at the wrapped indices; validity = the source's AND in range."""
    src_rows = cols[0].size
    idx = np.asarray(idx, np.int64)
    wrapped = np.where(idx < 0, idx + src_rows, idx)  # negative indices count from the end
    inside = (wrapped >= 0) & (wrapped < src_rows)
    assert nullify or inside.all()
    assert out.num_columns() == len(cols) and out.num_rows() == len(idx)
    at = np.where(inside, wrapped, 0)
    for c, (src, o) in enumerate(zip(cols, out.columns())):
        what = f"column {c}, {len(idx)} map rows"
        assert int(o.type().id()) == src.type_id and o.size() == len(idx) and o.offset() == 0, what
        got = R.raw_host_column(o)
        expect_valid = inside.copy()
        if src.valid is not None and src_rows:
            expect_valid &= np.take(src.valid[src.offset:], at)
        nulls = int((~expect_valid).sum())
        assert o.null_count() == nulls, f"{what}: null count"
        if src.valid is None and nulls == 0:
            assert got.valid is None, f"{what}: a mask on a column that had none and gained no null"
        elif len(idx):
            assert got.valid is not None and np.array_equal(got.valid, expect_valid), f"{what}: validity"
        if src_rows:
            expect = np.take(src.data[src.offset:], at)
            assert got.data[expect_valid].tobytes() == expect[expect_valid].tobytes(), f"{what}: data"
        else:
            assert not expect_valid.any()


def _nullify_map(rng, length, src_rows):
    """In-range indices of either sign with the out-of-range values -1 - src_rows, src_rows, INT32_MIN, INT32_MAX and the in-range
    edges -1, -src_rows at positions 0, 31, 32, 63, 64 and the last one, where the length allows."""
    idx = rng.integers(-max(src_rows, 3), max(src_rows, 3), length).astype(np.int64)  # (a source of no rows: nothing is in range)
    special = [-1, -src_rows, -src_rows - 1, src_rows, INT32_MIN, INT32_MAX]
    for k, pos in enumerate([0, 31, 32, 63, 64, length - 1]):
        if 0 <= pos < length:
            idx[pos] = special[k]
    if length > 70:  # every special value next to every kind of position once the map is long enough
        idx[65:71] = special[::-1]
    return idx


@pytest.mark.parametrize("length", LENGTHS)
def test_gather_nullify(source, length):
    cols, table = source
    idx = _nullify_map(np.random.default_rng(length), length, SRC_ROWS)
    _check(cols, _gather(table, idx, "nullify"), idx, nullify=True)


@pytest.mark.parametrize("length", LENGTHS)
def test_gather_nullify_all_in_range(source, length):
    """No index out of range: a column without a mask comes back without nulls (and without a mask), nullable ones keep theirs."""
    cols, table = source
    idx = np.random.default_rng(1000 + length).integers(-SRC_ROWS, SRC_ROWS, length)
    out = _gather(table, idx, "nullify")
    _check(cols, out, idx, nullify=True)
    for src, o in zip(cols, out.columns()):
        if src.valid is None:
            assert o.null_count() == 0 and not o.nullable()


@pytest.mark.parametrize("length", LENGTHS)
def test_gather_dont_check(source, length):
    """In-range indices only, negative ones included (out of range is undefined under DONT_CHECK): nullable sources keep their
    nulls, the others come back without a mask."""
    cols, table = source
    idx = np.random.default_rng(2000 + length).integers(-SRC_ROWS, SRC_ROWS, length)
    if length:
        idx[0], idx[-1] = -SRC_ROWS, SRC_ROWS - 1
    out = _gather(table, idx, "dont_check")
    _check(cols, out, idx, nullify=False)
    for src, o in zip(cols, out.columns()):
        assert o.nullable() == (src.valid is not None and length > 0)


@pytest.mark.parametrize("policy", ["nullify", "dont_check"])
@pytest.mark.parametrize("length", [1, 33, 1025])
def test_gather_with_a_sliced_map(source, policy, length):
    """The map is rows [7, 7 + length) of its buffer; the seven rows before it would gather other rows."""
    cols, table = source
    rng = np.random.default_rng(3000 + length)
    idx = rng.integers(-SRC_ROWS, SRC_ROWS, length + 7)
    idx[:7] = [0, 1, 2, 3, 4, 5, 6]
    if policy == "nullify":
        idx[7] = SRC_ROWS
    _check(cols, _gather(table, idx, policy, offset=7), idx[7:], nullify=policy == "nullify")


@pytest.mark.parametrize("length", [1, 33, 1025])
def test_gather_from_a_source_of_no_rows(empty_source, length):
    """NULLIFY with nothing to gather from: every index is out of range, every output row of all nine types is null."""
    cols, table = empty_source
    idx = _nullify_map(np.random.default_rng(length), length, 0)
    out = _gather(table, idx, "nullify")
    _check(cols, out, idx, nullify=True)
    for o in out.columns():
        assert o.null_count() == length and not o.to_numpy()[1].any()


@pytest.mark.parametrize("policy", ["nullify", "dont_check"])
def test_gather_with_a_map_of_no_rows(source, policy):
    """Nine empty columns of the source's types."""
    cols, table = source
    out = _gather(table, np.zeros(0, np.int32), policy)
    assert out.num_columns() == 9 and out.num_rows() == 0
    for src, o in zip(cols, out.columns()):
        assert int(o.type().id()) == src.type_id and o.size() == 0 and o.null_count() == 0
