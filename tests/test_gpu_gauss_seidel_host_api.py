"""Runs the C++ drop-in header test of multicolor Gauss-Seidel (kokkos-kernels_amd/host/tests/test_gauss_seidel_drop_in.cpp) on the GPU:
the three apply functions over KokkosKernelsHandle::create_gs_handle on a small lattice matrix against a sweep computed in the
program, a rank-2 LayoutLeft view, the given_inverse_diagonal overload, get_point_gs_handle()->set_long_row_threshold,
destroy_gs_handle, and the KokkosSparse::Experimental:: names."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kokkos-kernels_amd", "host", "tests", "test_gauss_seidel_drop_in")


@pytest.mark.gpu
def test_cpp_gauss_seidel_drop_in_headers():
    assert os.path.exists(EXE), "build it with __graft_entry__.build() (make -C kokkos-kernels_amd/host)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_gauss_seidel_drop_in_headers_build():
    """CPU-side: the headers compile and link against libkkamd.so (no GPU needed to build)."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kokkos-kernels_amd", "host"), "-s", "tests/test_gauss_seidel_drop_in"])
    assert os.path.exists(EXE)
