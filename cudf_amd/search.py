"""pylibcudf.search mirror (reference python/pylibcudf/pylibcudf/search.pyx: lower_bound, upper_bound) over cudf::lower_bound and
cudf::upper_bound (include/cudf/search.hpp). contains is not served."""
import ctypes as C

from . import _lib
from .column import Column, Table, _stream_ptr
from .sorting import _orders


def _bound(haystack: Table, needles: Table, column_order, null_precedence, upper, stream):
    out = C.c_void_p()
    _lib.check(_lib.load().cudf_amd_search_bound(haystack._views(), haystack.num_columns(), needles._views(), needles.num_columns(),
                                                 *_orders(column_order, null_precedence), 1 if upper else 0, _stream_ptr(stream),
                                                 C.byref(out)))
    return Table._from_handle(out, stream).columns()[0]


def lower_bound(haystack: Table, needles: Table, column_order=None, null_precedence=None, stream=None, mr=None) -> Column:
    """For each row of `needles`, the number of rows of the sorted `haystack` that compare less than it: the first position at
    which it can be inserted. One INT32 Column. An empty `column_order` means ASCENDING and an empty `null_precedence`
    NullOrder.BEFORE for every column."""
    return _bound(haystack, needles, column_order, null_precedence, False, stream)


def upper_bound(haystack: Table, needles: Table, column_order=None, null_precedence=None, stream=None, mr=None) -> Column:
    """As lower_bound, with the rows that compare less than or equal to the needle: the last position at which it can be inserted."""
    return _bound(haystack, needles, column_order, null_precedence, True, stream)
