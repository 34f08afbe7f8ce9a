"""Runs the C++ drop-in header test of ParILUT (kokkos-kernels_amd/host/tests/test_par_ilut_drop_in.cpp) on the GPU:
KokkosSparse::Experimental::par_ilut_symbolic / par_ilut_numeric over KokkosKernelsHandle::create_par_ilut_handle on the reference's 4 x 4
fixture (nnzL, nnzU, the expected factors, the six views resized), then par_ilut, LUPrec and gmres on a small diagonally dominant matrix."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kokkos-kernels_amd", "host", "tests", "test_par_ilut_drop_in")


@pytest.mark.gpu
def test_cpp_par_ilut_drop_in_headers():
    assert os.path.exists(EXE), "build it with __graft_entry__.build() (make -C kokkos-kernels_amd/host)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_par_ilut_drop_in_headers_build():
    """CPU-side: the headers compile and link against libkkamd.so (no GPU needed to build)."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kokkos-kernels_amd", "host"), "-s", "tests/test_par_ilut_drop_in"])
    assert os.path.exists(EXE)
