"""pylibcudf.sorting mirror (reference python/pylibcudf/pylibcudf/sorting.pyx: sorted_order, stable_sorted_order, sort, stable_sort,
sort_by_key, stable_sort_by_key, is_sorted, rank) over cudf::sorted_order and its siblings (include/cudf/sorting.hpp)."""
import ctypes as C

from . import _lib
from .aggregation import RankMethod
from .column import Column, Table, _stream_ptr
from .types import NullOrder, NullPolicy, Order


def _orders(column_order, null_precedence):
    """The two order lists as (array, length) pairs; an empty list selects the default of every column."""
    o = [int(Order(x)) for x in (column_order or [])]
    p = [int(NullOrder(x)) for x in (null_precedence or [])]
    return (C.c_int32 * max(1, len(o)))(*o), len(o), (C.c_int32 * max(1, len(p)))(*p), len(p)


def _sorted_order(input: Table, column_order, null_precedence, stable, stream):
    out = C.c_void_p()
    _lib.check(_lib.load().cudf_amd_sorted_order(input._views(), input.num_columns(), *_orders(column_order, null_precedence),
                                                 1 if stable else 0, _stream_ptr(stream), C.byref(out)))
    return Table._from_handle(out, stream).columns()[0]


def _sort_by_key(values: Table, keys: Table, column_order, null_precedence, stable, stream):
    out = C.c_void_p()
    _lib.check(_lib.load().cudf_amd_sort_by_key(values._views(), values.num_columns(), keys._views(), keys.num_columns(),
                                                *_orders(column_order, null_precedence), 1 if stable else 0, _stream_ptr(stream),
                                                C.byref(out)))
    return Table._from_handle(out, stream)


def sorted_order(source_table: Table, column_order=None, null_precedence=None, stream=None, mr=None) -> Column:
    """The row indices of `source_table` in lexicographic order, one INT32 Column. An empty `column_order` means ASCENDING and an
    empty `null_precedence` NullOrder.BEFORE for every column."""
    return _sorted_order(source_table, column_order, null_precedence, False, stream)


def stable_sorted_order(source_table: Table, column_order=None, null_precedence=None, stream=None, mr=None) -> Column:
    """As sorted_order; rows that compare equal keep their input order."""
    return _sorted_order(source_table, column_order, null_precedence, True, stream)


def sort(source_table: Table, column_order=None, null_precedence=None, stream=None, mr=None) -> Table:
    """The rows of `source_table` in lexicographic order."""
    return _sort_by_key(source_table, source_table, column_order, null_precedence, False, stream)


def stable_sort(source_table: Table, column_order=None, null_precedence=None, stream=None, mr=None) -> Table:
    """As sort; rows that compare equal keep their input order."""
    return _sort_by_key(source_table, source_table, column_order, null_precedence, True, stream)


def sort_by_key(values: Table, keys: Table, column_order=None, null_precedence=None, stream=None, mr=None) -> Table:
    """The rows of `values` in the lexicographic order of the rows of `keys`."""
    return _sort_by_key(values, keys, column_order, null_precedence, False, stream)


def stable_sort_by_key(values: Table, keys: Table, column_order=None, null_precedence=None, stream=None, mr=None) -> Table:
    """As sort_by_key; rows whose keys compare equal keep their input order."""
    return _sort_by_key(values, keys, column_order, null_precedence, True, stream)


def is_sorted(tbl: Table, column_order=None, null_precedence=None, stream=None) -> bool:
    """Whether no row of `tbl` is lexicographically less than its predecessor."""
    out = C.c_int32(0)
    _lib.check(_lib.load().cudf_amd_is_sorted(tbl._views(), tbl.num_columns(), *_orders(column_order, null_precedence),
                                              _stream_ptr(stream), C.byref(out)))
    return bool(out.value)


def rank(column: Column, method, column_order, null_handling, null_precedence, percentage, stream=None) -> Column:
    """The rank of every element of `column` in its stable sorted order, from 1: RankMethod FIRST, AVERAGE, MIN, MAX or DENSE
    among tied rows. FLOAT64 for AVERAGE or with `percentage` (rank / count), else INT32. NullPolicy.EXCLUDE keeps the column's
    validity; NullPolicy.INCLUDE ranks the nulls and returns no mask."""
    out = C.c_void_p()
    view = column._view()
    _lib.check(_lib.load().cudf_amd_rank(C.byref(view), int(RankMethod(method)), int(Order(column_order)),
                                         int(NullPolicy(null_handling)), int(NullOrder(null_precedence)), 1 if percentage else 0,
                                         _stream_ptr(stream), C.byref(out)))
    return Table._from_handle(out, stream).columns()[0]
