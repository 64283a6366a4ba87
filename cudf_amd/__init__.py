"""cudf_amd — MI355X-native (gfx950, hand-written HIP) hash-groupby / hash-join behind the libcudf API.

Python layer = a pylibcudf-shaped host mirror (Column, Table, groupby.GroupBy, join.inner_join, stream_compaction.distinct /
drop_nulls / drop_nans / apply_boolean_mask / apply_deletion_mask / unique / unique_count, ...) over the
C ABI of cudf_amd/lib/libcudf_amd.so. The shared library is the product; importing this package without it
fails (no CPU fallback)."""
from . import (_lib, aggregation, groupby, join, merge, partitioning, reduce, search, sorting, stream_compaction,  # noqa: F401
               types)
from .column import Column, Table  # noqa: F401
from .types import (DataType, DuplicateKeepOption, NanEquality, NanPolicy, NullEquality, NullOrder, NullPolicy, Order,  # noqa: F401
                    Sorted, TypeId)

__version__ = "0.1.0"
