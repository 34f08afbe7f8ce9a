"""KokkosSparse::Experimental::spgemm_jacobi under the SIMT emulator: kk_spgemm.hip compiled by g++ against kk_emu.h.  The library is the
one tests/emu/mis2.mk builds (tests/emu/Makefile's objects plus the MIS-2 unit), because two operands are tentative prolongators of
graph_mis2_aggregate.  Cases and checks: tests/spgemm_jacobi_cases.py -- structure and values `==` the definition on exactly representable
inputs, bit for bit the documented composition and the rounding bound on rounded ones, every lane width and both forms of the epilogue,
special values, statuses, the row-partitioned form, the smoothed prolongator."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np
import pytest

import kk_loader
import spgemm_jacobi_cases as jc
from emu import emu_backend

HERE = os.path.dirname(os.path.abspath(emu_backend.__file__))
SO = os.path.join(HERE, "libkkamd_emu_mis2.so")

OPERANDS = ("lat27_squared", "lat7_prolongator", "rmat_squared", "unsorted_B", "diagonal_A")


@pytest.fixture(scope="module")
def emu():
    kk = kk_loader.load()
    with open(emu_backend.LOCK, "w") as lk:               # the lock emu_backend.build() takes: the objects are shared
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", HERE, "-f", "mis2.mk", "-s", "libkkamd_emu_mis2.so"])
    lib = kk._capi.bind(C.CDLL(SO))
    return kk, kk.Backend(lib, lambda n, dt: np.zeros(int(n), dtype=dt), lambda a: None if a is None else a.ctypes.data,
                          lambda: None, lambda a: a, lambda a: np.array(a, copy=True), "emu")


@pytest.fixture(scope="module")
def operands(emu):
    return jc.exact_operands(*emu)


def test_the_library_exports_the_entry_points(emu):
    kk, be = emu
    assert hasattr(be.lib, "kkamd_spgemm_jacobi") and hasattr(be.lib, "kkamd_dist_spgemm_jacobi") and hasattr(kk, "spgemm_jacobi")


@pytest.mark.parametrize("name", OPERANDS)
@pytest.mark.parametrize("odt,vdt", jc.TYPE_GRID, ids=lambda t: np.dtype(t).name)
def test_exactly_the_definition(emu, operands, name, odt, vdt):
    kk, be = emu
    jc.check_exact(kk, be, name, *operands[name], odt, vdt, expect_fast=name not in ("unsorted_B", "lat27_squared"))


@pytest.mark.parametrize("name", OPERANDS)
@pytest.mark.parametrize("odt,vdt", jc.TYPE_GRID[:2], ids=lambda t: np.dtype(t).name)
def test_the_documented_composition_bit_for_bit_and_the_rounding_bound(emu, operands, name, odt, vdt):
    kk, be = emu
    share, bits = jc.check_rounded(kk, be, name, *operands[name], odt, vdt)
    assert share <= 1.0 and bits


@pytest.mark.parametrize("lanes", jc.WIDTHS)
def test_rows_of_b_under_every_lane_width(emu, lanes):
    kk, be = emu
    jc.check_widths(kk, be, lanes, np.int64 if lanes in (2, 16) else np.int32, np.float32 if lanes in (4, 16) else np.float64)


@pytest.mark.parametrize("odt,vdt", jc.TYPE_GRID[:2], ids=lambda t: np.dtype(t).name)
def test_bisection_of_rows_of_c_of_every_length(emu, odt, vdt):
    kk, be = emu
    jc.check_bisection(kk, be, odt, vdt)


def test_the_form_of_the_epilogue(emu):
    jc.check_forms(*emu)


def test_empty_operands(emu):
    jc.check_empty(*emu)


@pytest.mark.parametrize("odt,vdt", jc.TYPE_GRID[:2], ids=lambda t: np.dtype(t).name)
def test_special_values(emu, odt, vdt):
    kk, be = emu
    jc.check_special(kk, be, odt, vdt)


def test_statuses(emu):
    jc.check_statuses(*emu)


def test_row_partitioned(emu):
    jc.check_dist(*emu)


def test_smoothed_prolongator(emu):
    jc.check_use(*emu)
