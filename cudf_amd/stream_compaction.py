"""pylibcudf.stream_compaction mirror (reference python/pylibcudf/pylibcudf/stream_compaction.pyx: distinct, distinct_indices,
stable_distinct) over cudf::distinct (include/cudf/stream_compaction.hpp)."""
import ctypes as C

from . import _lib
from .column import Column, Table, _stream_ptr
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
