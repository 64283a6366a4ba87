"""The row-multiset checker of the partition / shuffle / gather GPU tests (tests/partition_reference.py) on the CPU: it accepts an
output built from the oracle's own hash_partition order with np.take, and rejects that output once one row sits in a neighbouring
partition, two values of one column are swapped, one validity bit is flipped, a -0.0 became +0.0, or one row overwrote another.
No GPU: this is what lets a green GPU test mean something."""
import copy

import numpy as np
import pytest

import partition_reference as R
from oracle.oracle import HostColumn

N, NPARTS = 20_000, 7


@pytest.fixture(scope="module")
def split(oracle):
    """(source columns, partition of every source row, output columns in the oracle's order, NPARTS + 1 offsets)."""
    cols = R.mover_table(N, seed=3)
    part, starts, order = oracle.hash_partition([cols[c] for c in R.HASHED], NPARTS)
    out = []
    for c in cols:
        data = np.take(c.data[c.offset:], order)
        valid = None if c.valid is None else np.take(c.valid[c.offset:], order)
        out.append(HostColumn(data, valid))
    offsets = np.append(starts, N).astype(np.int64)
    assert np.array_equal(part[order], R.partition_of_offsets(offsets, N))  # (the oracle's three outputs agree with each other)
    return cols, part, out, offsets


def corrupted(out):
    return [copy.deepcopy(c) for c in out]


def rejected(split, out, offsets):
    cols, part, _, _ = split
    with pytest.raises(AssertionError, match="rows differ"):
        R.assert_same_rows(cols, part, out, offsets)


def test_table_has_the_edges_the_checker_is_for():
    cols = R.mover_table(N, seed=3)
    assert [c.data.dtype.itemsize for c in cols] == [8, 4, 1, 2, 8, 1] and (cols[0].offset, cols[3].offset) == (13, 5)
    assert all(c.size == N for c in cols) and 0 < cols[0].null_count < N and 0 < cols[3].null_count < N
    bits = cols[4].data.view(np.uint64)
    for pattern in (R.NAN_A, R.NAN_B, -0.0, 0.0):
        assert (bits == np.array([pattern], np.float64).view(np.uint64)[0]).sum() > 100
    assert set(np.unique(cols[5].data)) == {0, 1, 2}


def test_accepts_the_oracles_own_partition(split):
    cols, part, out, offsets = split
    R.assert_same_rows(cols, part, out, offsets)
    # (and the order inside a partition is free: the scatter kernels rank rows with LDS atomics)
    rng = np.random.default_rng(0)
    perm = np.concatenate([offsets[p] + rng.permutation(offsets[p + 1] - offsets[p]) for p in range(NPARTS)])
    shuffled = [HostColumn(c.data[perm], None if c.valid is None else c.valid[perm]) for c in out]
    R.assert_same_rows(cols, part, shuffled, offsets)


def test_rows_that_tie_on_the_leading_key_are_ordered_by_their_fields(split, monkeypatch):
    """With a leading key that ties every row, the order is np.lexsort by (partition, validity and bits of every column) alone: the
    same verdicts."""
    cols, part, out, offsets = split
    monkeypatch.setattr(R, "mix", lambda words: (words[0] >> np.uint64(32)) & np.uint64(1))
    R.assert_same_rows(cols, part, out, offsets)
    monkeypatch.setattr(R, "mix", lambda words: np.zeros(len(words[0]), np.uint64))
    by_fields = R.sorted_rows(cols, part)
    words = R.packed_rows(cols, part)
    assert np.array_equal(by_fields, np.stack([w[np.lexsort(words[::-1])] for w in words], axis=1))
    R.assert_same_rows(cols, part, out, offsets)
    bad = corrupted(out)
    bad[2].data[5], bad[2].data[6] = 1, 2
    assert (out[2].data[5], out[2].data[6]) != (1, 2)
    rejected(split, bad, offsets)


def test_packing_is_a_bijection_of_the_fields():
    """Two rows that differ in one bit of one field differ in the packed words, whichever field it is (nothing is shifted out)."""
    base = [HostColumn(np.zeros(1, np.int64), np.ones(1, bool)), HostColumn(np.zeros(1, np.int32)), HostColumn(np.zeros(1, np.int8)),
            HostColumn(np.zeros(1, np.int16), np.ones(1, bool)), HostColumn(np.zeros(1, np.float64)), HostColumn(np.zeros(1, np.uint8))]
    zero = np.stack(R.packed_rows(base, [0]))
    seen = {zero.tobytes()}
    for c, col in enumerate(base):
        for bit in range(8 * col.data.dtype.itemsize):
            cols = corrupted(base)
            cols[c].data.view(f"u{col.data.dtype.itemsize}")[0] = 1 << bit
            seen.add(np.stack(R.packed_rows(cols, [0])).tobytes())
    for bit in range(32):
        seen.add(np.stack(R.packed_rows(base, [1 << bit])).tobytes())
    for c in (0, 3):
        cols = corrupted(base)
        cols[c].valid[0] = False
        seen.add(np.stack(R.packed_rows(cols, [0])).tobytes())
    assert len(seen) == 1 + (64 + 32 + 8 + 16 + 64 + 8) + 32 + 2


def test_rejects_a_row_moved_to_the_neighbouring_partition(split):
    cols, part, out, offsets = split
    moved = offsets.copy()
    moved[3] -= 1  # the last row of partition 2 now counts as the first of partition 3
    assert moved[3] > moved[2]
    rejected(split, out, moved)


def test_rejects_two_values_swapped_within_one_column(split):
    cols, part, out, offsets = split
    for c in range(len(out)):
        bad = corrupted(out)
        d = bad[c].data
        v = np.ones(len(d), bool) if bad[c].valid is None else bad[c].valid
        i = int(offsets[1])  # the first row of partition 1, and the next valid row of the same partition with other bits
        assert v[i]
        j = next(j for j in range(i + 1, int(offsets[2])) if v[j] and d[j].tobytes() != d[i].tobytes())
        d[i], d[j] = d[j].copy(), d[i].copy()
        rejected(split, bad, offsets)


def test_rejects_one_flipped_validity_bit(split):
    cols, part, out, offsets = split
    for c in (0, 3):
        for to in (False, True):
            bad = corrupted(out)
            i = int(np.nonzero(bad[c].valid != to)[0][17])
            bad[c].valid[i] = to
            rejected(split, bad, offsets)


def test_rejects_a_negative_zero_turned_positive(split):
    cols, part, out, offsets = split
    bad = corrupted(out)
    i = int(np.nonzero(bad[4].data.view(np.uint64) == 1 << 63)[0][0])
    bad[4].data[i] = 0.0
    assert out[4].data[i] == bad[4].data[i]  # (equal as numbers: only the bit pattern tells)
    rejected(split, bad, offsets)
    # the same for the payload of a NaN
    bad = corrupted(out)
    i = int(np.nonzero(bad[4].data.view(np.uint64) == np.array([R.NAN_A]).view(np.uint64)[0])[0][0])
    bad[4].data[i] = R.NAN_B
    rejected(split, bad, offsets)


def test_rejects_one_row_duplicated_over_another(split):
    cols, part, out, offsets = split
    bad = corrupted(out)
    i = int(offsets[4])
    for c in bad:  # row i + 1 := row i, every column and its validity (each column on its own still looks plausible)
        c.data[i + 1] = c.data[i]
        if c.valid is not None:
            c.valid[i + 1] = c.valid[i]
    rejected(split, bad, offsets)


def test_rejects_a_wrong_shape(split):
    cols, part, out, offsets = split
    with pytest.raises(AssertionError):
        R.assert_same_rows(cols, part, out[:-1], offsets)
    with pytest.raises(AssertionError):
        R.assert_same_rows(cols, part, out, offsets[:-1])
    with pytest.raises(AssertionError):
        R.assert_same_rows(cols, part, [HostColumn(c.data[:-1], None if c.valid is None else c.valid[:-1]) for c in out], offsets)
