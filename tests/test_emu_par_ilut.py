"""ParILUT under the SIMT emulator: kk_par_ilut.hip compiled by g++ against kk_emu.h (tests/emu/par_ilut.mk, which includes
tests/emu/Makefile and adds the unit; the product and the transposes run through kk_spgemm.hip and kk_util.hip of the shared objects) --
the steps bit for bit on exact inputs over both offset types, both value types and every lane count, the radix select against
numpy.partition, the whole loop against the restated reference loop within the measured tolerance, error statuses.  Cases at emulator
size (tests/par_ilut_cases.py, small=True)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np
import pytest

import kk_loader
import par_ilut_cases as pc
from emu import emu_backend

HERE = os.path.dirname(os.path.abspath(emu_backend.__file__))
SO = os.path.join(HERE, "libkkamd_emu_par_ilut.so")
_BACKEND = None
LANES = (1, 2, 4, 8, 16, 32, 64)


def backend():
    global _BACKEND
    if _BACKEND is None:
        kk = kk_loader.load()
        with open(emu_backend.LOCK, "w") as lk:               # the lock emu_backend.build() takes: the objects are shared
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-C", HERE, "-f", "par_ilut.mk", "-s", "libkkamd_emu_par_ilut.so"])
        lib = kk._capi.bind(C.CDLL(SO))
        _BACKEND = kk.Backend(lib, lambda n, dt: np.zeros(int(n), dtype=dt), lambda a: None if a is None else a.ctypes.data,
                              lambda: None, lambda a: a, lambda a: np.array(a, copy=True), "emu")
    return kk_loader.load(), _BACKEND


CASES = pc.loop_cases(True)


def test_cases_meet_the_condition_on_the_cpu():
    """no rounding decides a pattern or the stop: float32, float64, longdouble and 8 term orders agree (par_ilut_cases.analysed)"""
    for case in CASES:
        out = pc.analysed(case)
        assert set(out) == {np.float64, np.float32}
    assert pc.analysed(CASES[6])[np.float64][0].num_iters >= 2
    for kind in ("band", "arrow"):
        pc.exact_inputs(kind)


def test_reference_fixture():
    pc.check_fixture(*backend())


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("kind", ["band", "arrow"])
def test_steps_bit_for_bit(kind, lanes):
    kk, be = backend()
    for offset_dtype, dtype in ((np.int32, np.float64), (np.int64, np.float32), (np.int32, np.float32), (np.int64, np.float64)):
        pc.check_steps(kk, be, kind, offset_dtype, dtype, lanes)


@pytest.mark.parametrize("count", [1500, 5000])
def test_select_equals_numpy_partition(count):
    kk, be = backend()
    assert count < 2048 or count > 2 * 2048                   # below one workgroup's share; more than one workgroup histograms
    for dtype in (np.float64, np.float32):
        pc.check_select(kk, be, count, dtype)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_whole_loop_matches_reference_loop(case):
    kk, be = backend()
    pc.check_loop(kk, be, case, np.int32, np.float64)
    pc.check_loop(kk, be, case, np.int64, np.float32)


@pytest.mark.parametrize("lanes", [1, 64])
def test_whole_loop_other_lane_counts(lanes):
    kk, be = backend()
    for case in (CASES[7], CASES[9]):                          # recipe d and the arrow: staged and unstaged L rows
        pc.check_loop(kk, be, case, np.int32, np.float64, lanes)


def test_case_shapes():
    """the cases reach the paths they are meant for"""
    kk, be = backend()
    f = pc.Factored(kk, be, CASES[9])
    assert f.ih.get("lanes_in_use") == 4 and 130 > f.ih.get("stage_entries_per_lane") * 4       # the arrow's last row works in global memory
    f.close()
    f = pc.Factored(kk, be, CASES[6])
    assert f.ih.get("lanes_in_use") == 8
    f.close()
    g = pc.analysed(CASES[11])[np.float64][0]
    assert g.U[0][0] == 0 and all(g.L[i][0] == CASES[11].rows[i][0] for i in (1, 2, 4))          # u_diag == 0: the entries stay as they were
    h01, h30 = pc.analysed(CASES[12])[np.float64][0], pc.analysed(CASES[13])[np.float64][0]
    assert sum(len(r) for r in h01.L) == 60 and sum(len(r) for r in h30.L) > h30.nnzL and h30.l_threshold < h01.l_threshold
    assert pc.analysed(CASES[14])[np.float64][0].num_iters == 5 and pc.analysed(CASES[14])[np.float64][0].end_rel_res == 0


def test_error_statuses():
    pc.check_statuses(*backend())


def test_repeated_numeric_with_new_values():
    pc.check_repeated_numeric(*backend())


def test_verbose_prints_the_reference_lines(capfd):
    kk, be = backend()
    f = pc.Factored(kk, be, CASES[0])
    f.ih.set_verbose(True)
    f.numeric(np.float64)
    out = capfd.readouterr().out
    assert "Starting PARILUT with..." in out and "Completed itr 3, residual is: " in out and "PAR_ILUT stopped in 4 iterations with residual" in out
    f.close()
