"""pylibcudf.merge mirror (reference python/pylibcudf/pylibcudf/merge.pyx: merge) over cudf::merge (include/cudf/merge.hpp)."""
import ctypes as C

from . import _lib
from .column import Table, _stream_ptr
from .sorting import _orders


def merge(tables_to_merge, key_cols, column_order, null_precedence=None, stream=None, mr=None) -> Table:
    """Every row of the sorted `tables_to_merge` in one Table sorted on the columns `key_cols`. `column_order` has one entry per key
    column (an empty list does not mean ascending here); an empty `null_precedence` means NullOrder.BEFORE. Rows of one input whose
    keys compare equal keep their relative order."""
    tables = list(tables_to_merge)
    ncols = tables[0].num_columns() if tables else 0
    if any(t.num_columns() != ncols for t in tables):  # (the C call takes one column count for all tables)
        raise _lib.CudfAmdError("Mismatched number of columns")
    views = [t._views() for t in tables]
    ptrs = (C.POINTER(_lib.ColumnView) * max(1, len(views)))(*[C.cast(v, C.POINTER(_lib.ColumnView)) for v in views])
    keys = [int(k) for k in key_cols]
    out = C.c_void_p()
    _lib.check(_lib.load().cudf_amd_merge(ptrs, len(tables), ncols, (C.c_int32 * max(1, len(keys)))(*keys), len(keys),
                                          *_orders(column_order, null_precedence), _stream_ptr(stream), C.byref(out)))
    return Table._from_handle(out, stream)
