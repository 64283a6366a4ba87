"""cudf::rank's C++ header used directly (tests/cpp/rank_compat.cpp), as tests/test_sorting_cpp_api.py does for sorted_order.
CPU: it must compile and link; GPU: it must run the reference header's three documented examples."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rank_compat.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "rank_compat.bin")


def _build():
    lib_dir = os.path.join(ROOT, "cudf_amd", "lib")
    assert os.path.exists(os.path.join(lib_dir, "libcudf_amd.so")), "build the library first (__graft_entry__.build())"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++20", "-O1", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                           SRC, "-o", EXE, "-L", lib_dir, "-lcudf_amd", f"-Wl,-rpath,{lib_dir}"])


def test_rank_cpp_api_compiles_and_links():
    _build()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_rank_cpp_api_runs():
    if not os.path.exists(EXE):
        _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rank_compat OK" in out.stdout
