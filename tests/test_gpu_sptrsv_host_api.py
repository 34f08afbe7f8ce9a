"""Runs the C++ drop-in header test of the sparse triangular solve (kokkos-kernels_amd/host/tests/test_sptrsv_drop_in.cpp) on the GPU:
KokkosSparse::sptrsv_symbolic / sptrsv_solve over KokkosKernelsHandle::create_sptrsv_handle, with and without an execution space,
under the KokkosSparse::Experimental:: names too."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kokkos-kernels_amd", "host", "tests", "test_sptrsv_drop_in")


@pytest.mark.gpu
def test_cpp_sptrsv_drop_in_headers():
    assert os.path.exists(EXE), "build it with __graft_entry__.build() (make -C kokkos-kernels_amd/host)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_sptrsv_drop_in_headers_build():
    """CPU-side: the headers compile and link against libkkamd.so (no GPU needed to build)."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kokkos-kernels_amd", "host"), "-s", "tests/test_sptrsv_drop_in"])
    assert os.path.exists(EXE)
