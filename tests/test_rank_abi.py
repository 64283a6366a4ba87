"""CPU: cudf_amd_rank is declared in include/cudf_amd_c.h with the arguments the binding passes, exported by the built library and
bound in cudf_amd/_lib.py; the ABI number did not move; and the tile the GPU tests place their edges around is the kernels'."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "cudf_amd_c.h")) as f:
        return f.read()


def test_declared_in_the_c_header():
    m = re.search(r"cudf_amd_status\s+cudf_amd_rank\s*\(([^;]*)\)\s*;", _header())
    assert m, "cudf_amd_rank is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const cudf_amd_column_view* input", "int32_t method", "int32_t column_order", "int32_t null_handling",
                    "int32_t null_precedence", "int32_t percentage", "void* stream", "cudf_amd_table_t* out"]
    assert re.search(r"#define\s+CUDF_AMD_ABI_VERSION\s+4\b", _header())  # a new function does not bump it


def test_declared_in_the_cpp_header():
    with open(os.path.join(ROOT, "include", "cudf", "sorting.hpp")) as f:
        text = f.read()
    assert "#include <cudf/aggregation.hpp>" in text
    assert re.search(r"std::unique_ptr<column>\s+rank\(column_view const& input, rank_method method, order column_order, "
                     r"null_policy null_handling,\s+null_order null_precedence, bool percentage, stream_ref stream", text)


def test_exported_by_the_library():
    from cudf_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "cudf_amd_rank")
    assert _lib.load().cudf_amd_abi_version() == 4


def test_bound_in_the_python_module():
    import cudf_amd
    from cudf_amd import _lib
    res, args = _lib.SYMBOLS["cudf_amd_rank"]
    assert res is C.c_int and len(args) == 8
    assert args[1:6] == [C.c_int32] * 5
    assert callable(cudf_amd.sorting.rank)
    assert _lib.load().cudf_amd_rank.argtypes == args


def test_tile_constant_matches_the_kernels():
    """tests/test_rank_gpu.py puts its row counts and run edges around T: RANK_TILE of sorting_impl.hpp."""
    with open(os.path.join(ROOT, "cudf_amd", "csrc", "sorting", "sorting_impl.hpp")) as f:
        m = re.search(r"constexpr int RANK_TILE\s*=\s*(\d+);", f.read())
    import test_rank_gpu
    assert m and int(m.group(1)) == test_rank_gpu.T
