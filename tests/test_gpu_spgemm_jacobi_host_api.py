"""Runs the C++ drop-in header test of spgemm_jacobi (kokkos-kernels_amd/host/tests/test_spgemm_jacobi_drop_in.cpp) on the GPU:
KokkosSparse::Experimental::spgemm_jacobi after spgemm_symbolic for double / int and float / size_t, structure and values `==` the
definition summed in the program, dinv as a rank-2 view with one column and as a rank-1 view, the reference's exception text for a
transposed operand, a call before the symbolic phase, a row of A without its diagonal."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kokkos-kernels_amd", "host", "tests", "test_spgemm_jacobi_drop_in")


@pytest.mark.gpu
def test_cpp_spgemm_jacobi_drop_in_header():
    assert os.path.exists(EXE), "build it with __graft_entry__.build() (make -C kokkos-kernels_amd/host)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_spgemm_jacobi_drop_in_header_builds():
    """CPU-side: the header compiles and links against libkkamd.so (no GPU needed to build)."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kokkos-kernels_amd", "host"), "-s", "tests/test_spgemm_jacobi_drop_in"])
    assert os.path.exists(EXE)
