"""TEST INFRASTRUCTURE ONLY - a vectorised check that a partition / shuffle / gather moved whole rows: the multiset of
(partition, row) pairs of the output equals the source's, compared on raw bits. The membership check of
tests/test_partition_gpu.py::test_hash_partition builds Python tuples and skips partitions over 2000 rows; this one sorts packed
64-bit words with np.lexsort and skips nothing, so it can be used at the sizes where a scatter kernel runs its second tile.
tests/test_partition_reference.py proves on the CPU that it accepts a correct split and rejects five kinds of corruption. The check
reads nothing of the product (raw_host_column, the download the GPU tests feed it with, is the one function here that does).

A row is canonicalised column by column to (validity flag, raw bits as an unsigned integer of the column's width, zeroed where the
row is null). Floats are compared by bit pattern: a move keeps the payload of a NaN and the sign of a zero. The fields
(partition, v0, bits0, v1, bits1, ...) are packed side by side into 64-bit words - a bijection, so sorting the words is sorting by
the fields - and both sides are ordered with np.lexsort (sorted_rows); the sorted words must be equal."""
import numpy as np

from oracle.oracle import HostColumn


def as_host(c):
    """HostColumn, (data, valid_or_None) as cudf_amd.Column.to_numpy() returns it, or a bare array -> HostColumn."""
    if isinstance(c, HostColumn):
        return c
    if isinstance(c, tuple):
        return HostColumn(c[0], c[1])
    return HostColumn(c)


def canonical(c):
    """-> (bits: unsigned integers of the column's width, zero where null; valid: bool), the column's offset honoured."""
    c = as_host(c)
    data = c.data[c.offset:c.offset + c.size]
    bits = np.ascontiguousarray(data).view(np.dtype(f"u{data.dtype.itemsize}"))
    if c.valid is None:
        return bits, np.ones(c.size, bool)
    valid = c.valid[c.offset:c.offset + c.size]
    return np.where(valid, bits, bits.dtype.type(0)), valid


def packed_rows(cols, part):
    """The fields (part: 32 bits, then per column 1 validity bit and 8 * width data bits) packed into as few uint64 words as they
    fill, first field in the high bits of the first word. A field never straddles two words."""
    part = np.asarray(part)
    assert part.ndim == 1 and (len(part) == 0 or (part.min() >= 0 and part.max() < 2**32)), "partition ids must fit 32 bits"
    fields = [(part.astype(np.uint64), 32)]
    for c in cols:
        bits, valid = canonical(c)
        assert len(bits) == len(part), f"a column of {len(bits)} rows against {len(part)} partition ids"
        fields.append((valid.astype(np.uint64), 1))
        fields.append((bits.astype(np.uint64), 8 * bits.dtype.itemsize))
    words, cur, used = [], np.zeros(len(part), np.uint64), 0
    for values, width in fields:
        if used + width > 64:
            words.append(cur)
            cur, used = np.zeros(len(part), np.uint64), 0
        cur = cur | (values << np.uint64(64 - used - width))
        used += width
    words.append(cur)
    return words


def mix(words):
    """One 64-bit word per row, a function of all its packed words: the leading sort key. Rows that differ almost never share it."""
    key = np.zeros(len(words[0]), np.uint64)
    for w in words:
        key = (key ^ w) * np.uint64(0x9e3779b97f4a7c15)
        key ^= key >> np.uint64(29)
    return key


def sorted_rows(cols, part):
    """The packed rows in the order of np.lexsort by (mix of the row, partition, validity and bits of every column): one
    (rows, words) uint64 array. The leading key is a function of the other keys, so this is a total order on row contents and two
    row multisets are equal exactly if their sorted arrays are. It is there for speed alone: np.lexsort over five words takes
    seconds at 3M rows, an argsort of one word a tenth of that, and only the rows that tie on it (equal rows, or the rare distinct
    rows that share a mix) still go through np.lexsort with every key."""
    words = packed_rows(cols, part)
    key = mix(words)
    order = np.argsort(key)
    key = key[order]
    tie = key[1:] == key[:-1]
    if tie.any():
        in_tie = np.zeros(len(key), bool)
        in_tie[1:] |= tie
        in_tie[:-1] |= tie
        pos = np.nonzero(in_tie)[0]  # (runs of equal keys: each run is contiguous and the runs are in key order)
        rows = order[pos]
        order[pos] = rows[np.lexsort([w[rows] for w in words[::-1]] + [key[pos]])]  # (np.lexsort's LAST key is the primary one)
    return np.stack([w[order] for w in words], axis=1)


def partition_of_offsets(offsets, n):
    """P + 1 row offsets of the output's partitions (the last one is the row count) -> the partition of every output row."""
    offsets = np.asarray(offsets, dtype=np.int64)
    assert len(offsets) >= 2 and offsets[0] == 0 and offsets[-1] == n, f"offsets must run from 0 to the {n} rows"
    assert np.all(np.diff(offsets) >= 0), "offsets must never decrease"
    return np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))


def assert_same_rows(src_cols, src_part, out_cols, out_offsets, what="partition"):
    """Every source row, whole (all columns, validity included), is in the output exactly once and in the partition src_part names.
    src_cols: HostColumns (offsets honoured); src_part: the partition of every source row; out_cols: HostColumns or (data, valid)
    pairs; out_offsets: P + 1 row offsets of the output's partitions."""
    src_cols, out_cols = [as_host(c) for c in src_cols], [as_host(c) for c in out_cols]
    assert len(src_cols) == len(out_cols), f"{what}: {len(out_cols)} output columns for {len(src_cols)} source columns"
    n = len(src_part)
    for i, (s, o) in enumerate(zip(src_cols, out_cols)):
        assert s.data.dtype.itemsize == o.data.dtype.itemsize, f"{what}: column {i} changed its width"
        assert s.size == n and o.size == n, f"{what}: column {i} has {o.size} rows for {s.size} source rows ({n} partition ids)"
    out_part = partition_of_offsets(out_offsets, n)
    exp, got = sorted_rows(src_cols, src_part), sorted_rows(out_cols, out_part)
    if not np.array_equal(exp, got):
        bad = np.nonzero((exp != got).any(axis=1))[0]
        raise AssertionError(f"{what}: {len(bad)} of {n} rows differ once both sides are sorted by (partition, row bits); the first "
                             f"at sorted position {bad[0]}: expected words {[hex(int(x)) for x in exp[bad[0]]]}, got "
                             f"{[hex(int(x)) for x in got[bad[0]]]} (partition in the top 32 bits of the first word)")


def raw_host_column(col):
    """A device cudf_amd.Column -> HostColumn of its bytes as they are in memory (Column.to_numpy() turns BOOL8 bytes into
    True / False; a move must keep the byte, so BOOL8 is read as UINT8)."""
    from cudf_amd import Column
    from cudf_amd.types import DataType, TypeId
    if col.type().id() == TypeId.BOOL8:
        col = Column(DataType(TypeId.UINT8), col.size(), col.data_ptr(), col.null_mask_ptr(), col.null_count(), col.offset(),
                     owner=col, stream=col.stream())
    data, valid = col.to_numpy()
    return HostColumn(data, valid)


# ------------------------------------------------------------------ the table the row movers are tested on
NAN_A = np.array([0x7ff8000000000001], np.uint64).view(np.float64)[0]  # two NaN payloads: a move must keep either
NAN_B = np.array([0xfff4000000abcdef], np.uint64).view(np.float64)[0]
HASHED = [0, 1]  # the columns that decide the partition


def mover_table(n, seed=0):
    """n rows of: hashed nullable int64 sliced at offset 13, hashed int32; carried int8, nullable int16 sliced at offset 5, float64
    with NaNs of two payloads and both zeros, bool (bytes 0, 1 and 2: a move keeps the byte). Widths 1, 2, 4 and 8, a validity
    offset on a hashed and on a carried column."""
    rng = np.random.default_rng(seed)
    f = rng.integers(-4, 5, n) * 0.25
    kind = rng.integers(0, 16, n)
    f = np.where(kind == 0, NAN_A, np.where(kind == 1, NAN_B, np.where(kind == 2, -0.0, np.where(kind == 3, 0.0, f))))
    return [
        HostColumn(rng.integers(-(1 << 40), 1 << 40, n + 13, dtype=np.int64), rng.random(n + 13) > 0.1, "int64", offset=13),
        HostColumn(rng.integers(-50, 50, n).astype(np.int32), None, "int32"),
        HostColumn(rng.integers(-128, 128, n).astype(np.int8), None, "int8"),
        HostColumn(rng.integers(-(1 << 15), 1 << 15, n + 5).astype(np.int16), rng.random(n + 5) > 0.3, "int16", offset=5),
        HostColumn(f, None, "float64"),
        HostColumn(rng.integers(0, 3, n).astype(np.uint8), None, "bool"),
    ]
