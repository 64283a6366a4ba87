"""pylibcudf.groupby mirror (reference python/pylibcudf/pylibcudf/groupby.pyx:40-215): GroupByRequest,
GroupBy.aggregate / GroupBy.scan -> (keys Table, [results Table per request]) and GroupBy.replace_nulls -> (keys Table, Table).
scan and replace_nulls return their rows in group order: groups contiguous, input order inside a group."""
import ctypes as C
from enum import IntEnum

from . import _lib
from .column import Table, _stream_ptr
from .types import NullPolicy, Sorted


class HashPath(IntEnum):
    NONE = 0
    LDS_SINGLE_PASS = 1
    PARTITIONED_LDS = 2
    GLOBAL_TABLE = 3
    DENSE_DIRECT = 4
    SORT = 5


class GroupByRequest:
    def __init__(self, values, aggregations):
        self._values = values
        self._aggregations = list(aggregations)


class GroupBy:
    def __init__(self, keys: Table, null_handling: NullPolicy = NullPolicy.EXCLUDE,
                 keys_are_sorted: Sorted = Sorted.NO, column_order=None, null_precedence=None):
        self._keys = keys  # pinned, as pylibcudf does (groupby.pyx:143-145)
        self._null_handling = NullPolicy(null_handling)
        self._keys_are_sorted = Sorted(keys_are_sorted)
        self.last_path = HashPath.NONE

    def aggregate(self, requests, stream=None, mr=None):
        lib = _lib.load()
        reqs, keep = [], []
        for r in requests:
            reqs.append(_lib.AggregationRequest.of(r._values._view(), r._aggregations, keep))
        rarr = (_lib.AggregationRequest * max(1, len(reqs)))(*reqs)
        out_keys, out_res, path = C.c_void_p(), C.c_void_p(), C.c_int32(0)
        _lib.check(lib.cudf_amd_groupby_aggregate(self._keys._views(), self._keys.num_columns(),
                                                  int(self._null_handling), int(self._keys_are_sorted), rarr,
                                                  len(reqs), _stream_ptr(stream), C.byref(out_keys),
                                                  C.byref(out_res), C.byref(path)))
        self.last_path = HashPath(path.value)
        keys = Table._from_handle(out_keys, stream)
        flat = Table._from_handle(out_res, stream, ragged=True).columns()
        results, p = [], 0
        for r in requests:
            results.append(Table(flat[p:p + len(r._aggregations)], ragged=True))
            p += len(r._aggregations)
        return keys, results

    def _run(self, fn, requests, stream):
        lib = _lib.load()
        reqs, keep = [], []
        for r in requests:
            reqs.append(_lib.AggregationRequest.of(r._values._view(), r._aggregations, keep))
        rarr = (_lib.AggregationRequest * max(1, len(reqs)))(*reqs)
        out_keys, out_res = C.c_void_p(), C.c_void_p()
        _lib.check(getattr(lib, fn)(self._keys._views(), self._keys.num_columns(), int(self._null_handling),
                                    int(self._keys_are_sorted), rarr, len(reqs), _stream_ptr(stream), C.byref(out_keys),
                                    C.byref(out_res)))
        keys = Table._from_handle(out_keys, stream)
        flat = Table._from_handle(out_res, stream, ragged=True).columns()
        results, p = [], 0
        for r in requests:
            results.append(Table(flat[p:p + len(r._aggregations)], ragged=True))
            p += len(r._aggregations)
        return keys, results

    def scan(self, requests, stream=None, mr=None):
        """Grouped inclusive scans (pylibcudf GroupBy.scan): SUM, PRODUCT, MIN, MAX, COUNT and RANK."""
        return self._run("cudf_amd_groupby_scan", requests, stream)

    def replace_nulls(self, values: Table, replace_policies, stream=None, mr=None):
        """Grouped forward / backward fill (pylibcudf GroupBy.replace_nulls): one ReplacePolicy per column."""
        lib = _lib.load()
        pol = [int(p) for p in replace_policies]
        if len(pol) != values.num_columns():  # the C ABI takes one policy per column (reference groupby.cu:293-294)
            raise _lib.CudfAmdError("Size mismatch between num_columns and replace_policies.")
        parr = (C.c_int32 * max(1, len(pol)))(*pol)
        out_keys, out_vals = C.c_void_p(), C.c_void_p()
        _lib.check(lib.cudf_amd_groupby_replace_nulls(self._keys._views(), self._keys.num_columns(), int(self._null_handling),
                                                      int(self._keys_are_sorted), values._views(), values.num_columns(),
                                                      parr, _stream_ptr(stream), C.byref(out_keys), C.byref(out_vals)))
        return Table._from_handle(out_keys, stream), Table._from_handle(out_vals, stream)
