"""MIS-2, MIS-2 aggregation and explicit coarsening under the SIMT emulator: kk_mis2.hip compiled by g++ against kk_emu.h (tests/emu/mis2.mk,
which includes tests/emu/Makefile and adds the unit) -- the set and its rounds against the restated loops for both algorithms, labels and
aggregate counts for coarsen and aggregate, every lanes-per-vertex value, the distance-2 definition, the coarse graph with and without
compress, the inverse map, the host-synchronisation formula, error statuses, the empty graph.  Cases: tests/mis2_cases.py, small=True."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np
import pytest

import kk_loader
import mis2_cases as mc
from emu import emu_backend

HERE = os.path.dirname(os.path.abspath(emu_backend.__file__))
SO = os.path.join(HERE, "libkkamd_emu_mis2.so")
_BACKEND = None
SMALL = True


def backend():
    global _BACKEND
    if _BACKEND is None:
        kk = kk_loader.load()
        with open(emu_backend.LOCK, "w") as lk:               # the lock emu_backend.build() takes: the objects are shared
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-C", HERE, "-f", "mis2.mk", "-s", "libkkamd_emu_mis2.so"])
        lib = kk._capi.bind(C.CDLL(SO))
        _BACKEND = kk.Backend(lib, lambda n, dt: np.zeros(int(n), dtype=dt), lambda a: None if a is None else a.ctypes.data,
                              lambda: None, lambda a: a, lambda a: np.array(a, copy=True), "emu")
    return kk_loader.load(), _BACKEND


CASES = mc.all_cases(SMALL)


def test_case_shapes():
    mc.check_shapes(SMALL)


def test_the_library_exports_the_unit():
    kk, be = backend()
    assert all(hasattr(be.lib, name) for name in kk._capi.MIS2_EXPORTS)
    assert (kk._capi.MIS2_QUALITY, kk._capi.MIS2_FAST) == (0, 1)
    assert kk.mis2_algorithm_name("MIS2_FAST") == "MIS2_FAST"


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_set_and_its_rounds_match_the_restated_loops(case):
    kk, be = backend()
    mc.check_mis(kk, be, case, np.int64 if case.name in ("lat7", "ghosts") else np.int32)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_labels_match_the_restated_aggregation(case):
    kk, be = backend()
    mc.check_aggregation(kk, be, case, np.int64 if case.name in ("lat27", "selfloops") else np.int32)


@pytest.mark.parametrize("case", mc.all_cases(SMALL, ("ghosts", "selfloops", "hub")), ids=repr)
def test_no_output_depends_on_the_lanes_per_vertex(case):
    kk, be = backend()
    # hub: 206 rounds of one vertex each under MIS2_QUALITY, the other two cover it; ghosts runs all seven widths, the others the
    # widths of both ends and the middle (the GPU test runs all seven on every case)
    mc.check_lanes(kk, be, case, quality=case.name != "hub", lanes_values=mc.LANES if case.name == "ghosts" else (0, 1, 4, 16, 64))


@pytest.mark.parametrize("case", mc.all_cases(SMALL, ("ghosts", "selfloops", "ring", "hub")), ids=repr)
def test_explicit_coarsening_and_the_inverse_map(case):
    kk, be = backend()
    mc.check_coarsening(kk, be, case, np.int64 if case.name in ("ring", "ghosts") else np.int32)


def test_error_statuses():
    kk, be = backend()
    mc.check_statuses(kk, be, mc.all_cases(SMALL, ("lat7",))[0])


def test_empty_graph():
    kk, be = backend()
    mc.check_empty(kk, be)
