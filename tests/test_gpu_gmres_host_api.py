"""Runs the C++ drop-in header test of GMRES (kokkos-kernels_amd/host/tests/test_gmres_drop_in.cpp) on the GPU: gmres over
KokkosKernelsHandle::create_gmres_handle for two type pairs, CGS2 and MGS, MatrixPrec, LUPrec with exact factors (one iteration), a user's
subclass of Preconditioner reached through the callback kind, restarts, the handle's setters and reset_handle, the dimension check's
text and m <= 0."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kokkos-kernels_amd", "host", "tests", "test_gmres_drop_in")


@pytest.mark.gpu
def test_cpp_gmres_drop_in_headers():
    assert os.path.exists(EXE), "build it with __graft_entry__.build() (make -C kokkos-kernels_amd/host)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_gmres_drop_in_headers_build():
    """CPU-side: the headers compile and link against libkkamd.so (no GPU needed to build)."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kokkos-kernels_amd", "host"), "-s", "tests/test_gmres_drop_in"])
    assert os.path.exists(EXE)
