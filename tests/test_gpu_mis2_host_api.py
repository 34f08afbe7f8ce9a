"""Runs the C++ drop-in header test of the MIS-2 unit (kokkos-kernels_amd/host/tests/test_mis2_drop_in.cpp) on the GPU:
KokkosGraph::graph_d2_mis for both algorithms, graph_mis2_coarsen, graph_mis2_aggregate, mis2_algorithm_name, the deprecated
KokkosGraph::Experimental:: names, graph_explicit_coarsen and graph_explicit_coarsen_with_inverse_map on a 7-point lattice, for int and
size_t offsets, each checked in the program from its definition."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kokkos-kernels_amd", "host", "tests", "test_mis2_drop_in")


@pytest.mark.gpu
def test_cpp_mis2_drop_in_headers():
    assert os.path.exists(EXE), "build it with __graft_entry__.build() (make -C kokkos-kernels_amd/host)"
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout


def test_cpp_mis2_drop_in_headers_build():
    """CPU-side: the headers compile and link against libkkamd.so (no GPU needed to build)."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "kokkos-kernels_amd", "host"), "-s", "tests/test_mis2_drop_in"])
    assert os.path.exists(EXE)
