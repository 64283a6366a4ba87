"""The distinct and unique counts of pylibcudf (reference python/pylibcudf/pylibcudf/stream_compaction.pyx distinct_count,
unique_count) over cudf::distinct_count (include/cudf/reduction/distinct_count.hpp) and cudf::unique_count
(include/cudf/reduction/unique_count.hpp)."""
import ctypes as C

from . import _lib
from .column import Column, Table, _stream_ptr
from .types import NanPolicy, NullEquality, NullPolicy


def distinct_count(source: Column, null_handling: NullPolicy, nan_handling: NanPolicy, stream=None) -> int:
    """The distinct elements of `source`: null_handling INCLUDE counts null as a value, nan_handling NAN_IS_NULL counts NaN as
    null."""
    out = C.c_int32()
    _lib.check(_lib.load().cudf_amd_distinct_count_column(C.byref(source._view()), int(NullPolicy(null_handling)),
                                                          int(NanPolicy(nan_handling)), _stream_ptr(stream), C.byref(out)))
    return out.value


def distinct_count_table(source: Table, nulls_equal: NullEquality = NullEquality.EQUAL, stream=None) -> int:
    """The distinct rows of `source` (NaN equals NaN)."""
    out = C.c_int32()
    _lib.check(_lib.load().cudf_amd_distinct_count_table(source._views(), source.num_columns(),
                                                         1 if nulls_equal == NullEquality.EQUAL else 0, _stream_ptr(stream),
                                                         C.byref(out)))
    return out.value


def unique_count(source: Column, null_handling: NullPolicy, nan_handling: NanPolicy, stream=None) -> int:
    """The runs of equal consecutive elements of `source` (what a sorted column's distinct count is), nulls and NaNs counted as
    the policies say."""
    out = C.c_int32()
    _lib.check(_lib.load().cudf_amd_unique_count_column(C.byref(source._view()), int(NullPolicy(null_handling)),
                                                        int(NanPolicy(nan_handling)), _stream_ptr(stream), C.byref(out)))
    return out.value


def unique_count_table(source: Table, nulls_equal: NullEquality = NullEquality.EQUAL, stream=None) -> int:
    """The runs of equal consecutive rows of `source` (NaN equals NaN)."""
    out = C.c_int32()
    _lib.check(_lib.load().cudf_amd_unique_count_table(source._views(), source.num_columns(),
                                                       1 if nulls_equal == NullEquality.EQUAL else 0, _stream_ptr(stream),
                                                       C.byref(out)))
    return out.value
