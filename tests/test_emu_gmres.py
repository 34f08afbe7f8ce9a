"""Restarted GMRES under the SIMT emulator: kk_gmres.hip and kk_sptrsv.hip compiled by g++ against kk_emu.h (tests/emu/gmres.mk, which
includes tests/emu/Makefile and adds the two units) -- the kernels bit for bit against numpy in longdouble, fuse 0 against fuse 1, the
solver against the restated reference loop, the invariants, the three preconditioner kinds, errors and handle state.  Cases are cut to
emulator size (tests/gmres_cases.py, small=True); the LU factors come from numpy (the emulator library has no spiluk)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np
import pytest

import kk_loader
import gmres_cases as gc
from emu import emu_backend

HERE = os.path.dirname(os.path.abspath(emu_backend.__file__))
SO = os.path.join(HERE, "libkkamd_emu_gmres.so")
_BACKEND = None
SMALL = True


def backend():
    global _BACKEND
    if _BACKEND is None:
        kk = kk_loader.load()
        with open(emu_backend.LOCK, "w") as lk:               # the lock emu_backend.build() takes: the objects are shared
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-C", HERE, "-f", "gmres.mk", "-s", "libkkamd_emu_gmres.so"])
        lib = kk._capi.bind(C.CDLL(SO))
        _BACKEND = kk.Backend(lib, lambda n, dt: np.zeros(int(n), dtype=dt), lambda a: None if a is None else a.ctypes.data,
                              lambda: None, lambda a: a, lambda a: np.array(a, copy=True), "emu")
    return kk_loader.load(), _BACKEND


NAMES = [c.name for c in gc.cases(SMALL)]
EMU_N = (1, 63, 64, 65, 130)


def test_case_shapes():
    """the conditions on the cases, at both sizes, on the restated loop alone"""
    gc.check_case_shapes(True)
    gc.check_case_shapes(False)


# 1 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", gc.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n", EMU_N)
def test_kernels_bit_for_bit(n, dtype):
    kk, be = backend()
    for i, k in enumerate(gc.KERNEL_K if n <= 65 else (9, 50, 65)):
        gc.check_kernels_exact(kk, be, n, k, dtype, pick=((0, 3), (1, 2))[i % 2] if k not in (64, 65) else (0, 1, 2, 3))


@pytest.mark.parametrize("dtype", gc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_kernels_inf_nan(dtype):
    kk, be = backend()
    for fuse in (0, 1):
        gc.check_kernels_nonfinite(kk, be, dtype, fuse)


# 2 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", gc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_fuse_0_equals_fuse_1(dtype):
    kk, be = backend()
    for n, k in ((65, 9), (130, 17), (70, 64), (70, 65), (1, 1)):
        gc.check_fuse_equivalence(kk, be, n, k, dtype, runs=(0, 1, 1) if k != 9 else (0, 1, 0, 1))


# 3 and 4 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ortho", ["CGS2", "MGS"])
@pytest.mark.parametrize("dtype", gc.DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", NAMES)
def test_solver_against_the_restated_loop(name, dtype, ortho):
    kk, be = backend()
    r1, _ = gc.check_solver(kk, be, SMALL, name, dtype, ortho, fuse=1)
    if ortho == "MGS":                                                         # the knob "fuse" has no part in MGS
        return
    r0, _ = gc.check_solver(kk, be, SMALL, name, dtype, ortho, fuse=0, offset_dtype=np.int64, rows_per_group=64)
    if r1.cycles > 0 and gc.case(SMALL, name).n <= 64:                         # one group either way: the knob changes no bit
        assert r0.X.tobytes() == r1.X.tobytes() and (r1.last_fused, r0.last_fused) == (1, 0)


def test_fuse_changes_no_bit_of_a_solve():
    kk, be = backend()
    c = gc.case(SMALL, "conv2d-m10")
    for dtype in gc.DTYPES:
        tol = gc.reference(SMALL, c.name, dtype, "CGS2")[0]
        a, b = (gc.solve(kk, be, c, dtype, "CGS2", tol, fuse=f) for f in (0, 1))
        assert a.X.tobytes() == b.X.tobytes() and a.H.tobytes() == b.H.tobytes() and a.V.tobytes() == b.V.tobytes()
        assert a.launches > b.launches and a.host_syncs == b.host_syncs


# 5 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", gc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_preconditioners(dtype):
    kk, be = backend()
    gc.check_preconditioners(kk, be, SMALL, dtype)


# 6 ----------------------------------------------------------------------------------------------------------------------------------

def test_errors_and_state():
    kk, be = backend()
    gc.check_errors_and_state(kk, be, SMALL)
