"""pylibcudf.stream_compaction mirror (reference python/pylibcudf/pylibcudf/stream_compaction.pyx: distinct, distinct_indices,
stable_distinct, drop_nulls, drop_nans, apply_boolean_mask, apply_deletion_mask, unique, unique_count) over
include/cudf/stream_compaction.hpp and include/cudf/reduction/unique_count.hpp."""
import ctypes as C

from . import _lib
from .column import Column, Table, _stream_ptr
from .reduce import unique_count, unique_count_table  # noqa: F401
from .types import DuplicateKeepOption, NanEquality, NullEquality


def _flags(keep, nulls_equal, nans_equal):
    return (int(DuplicateKeepOption(keep)), 1 if nulls_equal == NullEquality.EQUAL else 0,
            1 if nans_equal == NanEquality.ALL_EQUAL else 0)


def _distinct(input: Table, keys, keep, nulls_equal, nans_equal, stable, stream):
    keys = [int(k) for k in keys]
    arr = (C.c_int32 * max(1, len(keys)))(*keys)
    out = C.c_void_p()
    _lib.check(_lib.load().cudf_amd_distinct(input._views(), input.num_columns(), arr, len(keys),
                                             *_flags(keep, nulls_equal, nans_equal), 1 if stable else 0, _stream_ptr(stream),
                                             C.byref(out)))
    return Table._from_handle(out, stream)


def distinct(input: Table, keys, keep: DuplicateKeepOption = DuplicateKeepOption.KEEP_ANY,
             nulls_equal: NullEquality = NullEquality.EQUAL, nans_equal: NanEquality = NanEquality.ALL_EQUAL, stream=None,
             mr=None) -> Table:
    """The rows of `input` whose key columns (indices `keys`) are distinct; which row of a set of equal rows survives follows
    `keep`. Row order unspecified (here: input order)."""
    return _distinct(input, keys, keep, nulls_equal, nans_equal, False, stream)


def stable_distinct(input: Table, keys, keep: DuplicateKeepOption = DuplicateKeepOption.KEEP_ANY,
                    nulls_equal: NullEquality = NullEquality.EQUAL, nans_equal: NanEquality = NanEquality.ALL_EQUAL, stream=None,
                    mr=None) -> Table:
    """As distinct, in input order."""
    return _distinct(input, keys, keep, nulls_equal, nans_equal, True, stream)


def distinct_indices(input: Table, keep: DuplicateKeepOption = DuplicateKeepOption.KEEP_ANY,
                     nulls_equal: NullEquality = NullEquality.EQUAL, nans_equal: NanEquality = NanEquality.ALL_EQUAL, stream=None,
                     mr=None) -> Column:
    """The surviving row indices of `input` (every column a key), one INT32 Column in ascending order."""
    out = C.c_void_p()
    _lib.check(_lib.load().cudf_amd_distinct_indices(input._views(), input.num_columns(), *_flags(keep, nulls_equal, nans_equal),
                                                     _stream_ptr(stream), C.byref(out)))
    return Table._from_handle(out, stream).columns()[0]


def _keyed(fn, input: Table, keys, *rest, stream=None):
    keys = [int(k) for k in keys]
    arr = (C.c_int32 * max(1, len(keys)))(*keys)
    out = C.c_void_p()
    _lib.check(fn(input._views(), input.num_columns(), arr, len(keys), *rest, _stream_ptr(stream), C.byref(out)))
    return Table._from_handle(out, stream)


def drop_nulls(source_table: Table, keys, keep_threshold=None, stream=None, mr=None) -> Table:
    """The rows of `source_table` with at least `keep_threshold` valid fields among the key columns (indices `keys`); None: all of
    them. Input order; every column is filtered."""
    return _keyed(_lib.load().cudf_amd_drop_nulls, source_table, keys, -1 if keep_threshold is None else int(keep_threshold),
                  stream=stream)


def drop_nans(source_table: Table, keys, keep_threshold=None, stream=None, mr=None) -> Table:
    """The rows of `source_table` with at least `keep_threshold` fields that are not NaN among the FLOAT32 / FLOAT64 key columns
    (a null counts as not NaN); None: all of them."""
    return _keyed(_lib.load().cudf_amd_drop_nans, source_table, keys, -1 if keep_threshold is None else int(keep_threshold),
                  stream=stream)


def _apply_mask(source_table: Table, mask: Column, deletion, stream):
    out = C.c_void_p()
    _lib.check(_lib.load().cudf_amd_apply_boolean_mask(source_table._views(), source_table.num_columns(), C.byref(mask._view()),
                                                       1 if deletion else 0, _stream_ptr(stream), C.byref(out)))
    return Table._from_handle(out, stream)


def apply_boolean_mask(source_table: Table, boolean_mask: Column, stream=None, mr=None) -> Table:
    """The rows of `source_table` whose element of the BOOL8 column `boolean_mask` is valid and true."""
    return _apply_mask(source_table, boolean_mask, False, stream)


def apply_deletion_mask(source_table: Table, deletion_mask: Column, stream=None, mr=None) -> Table:
    """The rows of `source_table` whose element of the BOOL8 column `deletion_mask` is valid and false."""
    return _apply_mask(source_table, deletion_mask, True, stream)


def unique(input: Table, keys, keep: DuplicateKeepOption, nulls_equal: NullEquality = NullEquality.EQUAL, stream=None,
           mr=None) -> Table:
    """Of every run of consecutive rows with equal key columns, the first (KEEP_FIRST, KEEP_ANY), the last (KEEP_LAST) or, for runs
    longer than one row, none (KEEP_NONE)."""
    return _keyed(_lib.load().cudf_amd_unique, input, keys, int(DuplicateKeepOption(keep)),
                  1 if nulls_equal == NullEquality.EQUAL else 0, stream=stream)
