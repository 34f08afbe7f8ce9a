"""Multicolor Gauss-Seidel under the SIMT emulator: kk_gauss_seidel.hip compiled by g++ against kk_emu.h (tests/emu/gauss_seidel.mk, which
includes tests/emu/Makefile and adds the unit) -- the colouring against the restated greedy colouring, exact sweeps over every knob,
launch counts, composition and rank-2 identities bit for bit, the local rounding bound, error statuses.  Cases are cut to emulator
size (tests/gauss_seidel_cases.py, small=True)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np
import pytest

import kk_loader
import gauss_seidel_cases as gc
import sptrsv_cases as tc
from emu import emu_backend

HERE = os.path.dirname(os.path.abspath(emu_backend.__file__))
SO = os.path.join(HERE, "libkkamd_emu_gauss_seidel.so")
_BACKEND = None
SMALL = True


def backend():
    global _BACKEND
    if _BACKEND is None:
        kk = kk_loader.load()
        with open(emu_backend.LOCK, "w") as lk:               # the lock emu_backend.build() takes: the objects are shared
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-C", HERE, "-f", "gauss_seidel.mk", "-s", "libkkamd_emu_gauss_seidel.so"])
        lib = kk._capi.bind(C.CDLL(SO))
        _BACKEND = kk.Backend(lib, lambda n, dt: np.zeros(int(n), dtype=dt), lambda a: None if a is None else a.ctypes.data,
                              lambda: None, lambda a: a, lambda a: np.array(a, copy=True), "emu")
    return kk_loader.load(), _BACKEND


CASES = gc.all_cases(SMALL)
DTYPES = (np.float64, np.float32)


def _status(fn):
    kk = kk_loader.load()
    with pytest.raises(kk.KkamdError) as e:
        fn()
    return e.value.status, str(e.value)


# 1 and 2 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=repr)
def test_colours_match_the_greedy_colouring(case):
    kk, be = backend()
    for offset_dtype in (np.int32, np.int64):
        for threshold in ((0, 64) if case.name == "e" else (0,)):
            sm = gc.Smoother(kk, be, case, "GS_DEFAULT", offset_dtype, threshold)
            gc.check_coloring(sm)
            sm.symbolic()                                   # a second symbolic call gives the same arrays
            gc.check_coloring(sm)
            sm.close()


def test_case_shapes():
    """the small cases reach the paths they are meant for"""
    kk, be = backend()
    c = gc.cases(SMALL)
    assert int(c["a"][0].colors.max()) == 1
    assert c["e"][0].row_len.max() > 64 + 64               # beyond one pass of 64 lanes
    sm = gc.Smoother(kk, be, c["e"][0], threshold=64)
    assert sm.gh.get("long_rows") == 3 and sm.gh.get("long_row_threshold") == 64
    sm.gh.set("chain_rows", 0)
    assert sm.gh.get("tail_launches") >= 1
    sm.close()
    assert c["f"][0].greedy[0].max() > 1 and (c["f"][0].entries <= c["f"][0].rows).all()
    assert c["g"][0].ncols == c["g"][0].n + 37 and (c["g"][0].entries >= c["g"][0].n).sum() > 20
    sm = gc.Smoother(kk, be, c["i"][0])
    assert sm.gh.get_num_colors() == 70 and sm.gh.get("max_level_rows") == 3
    assert (sm.gh.get("launches"), sm.gh.get("chain_launches"), sm.gh.get("chained_levels")) == (1, 1, 70)
    sm.gh.set("chain_levels", 2)
    assert sm.gh.get("launches") == 35
    sm.close()
    sm = gc.Smoother(kk, be, c["b"][0], "GS_PERMUTED")
    assert sm.gh.get_algorithm_type() == "GS_PERMUTED" and sm.gh.get("algorithm") == 1
    sm.close()


def test_supplied_colours_are_validated():
    kk, be = backend()
    gc.check_supplied_colours(kk, be, SMALL)


# 3 ----------------------------------------------------------------------------------------------------------------------------------

def test_the_generator_is_exact_under_the_restated_sweep():
    for case in gc.all_cases(SMALL, ("c", "e", "g")):
        for dtype in DTYPES:
            for direction in gc.DIRECTIONS:
                values, x0, y, x1 = case.exact(direction, 1.5)
                x = gc.reference_sweep(case, values.astype(dtype), x0.astype(dtype), y.astype(dtype), 1.5, direction, dtype)
                assert np.array_equal(x, x1.astype(dtype))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_exact_sweeps_default_knobs(case):
    kk, be = backend()
    for k, algo in enumerate(gc.ALGORITHMS):
        sm = gc.Smoother(kk, be, case, algo, (np.int32, np.int64)[k % 2])
        gc.check_exact(sm, DTYPES[k % 2], "forward", 1.0, numeric=False)      # apply runs the numeric phase of a fresh analysis itself
        for dtype in DTYPES:
            for direction in gc.DIRECTIONS:
                for omega in gc.OMEGAS:
                    gc.check_exact(sm, dtype, direction, omega)
                gc.check_exact(sm, dtype, direction, 1.0, zero_x=True)
        sm.close()


@pytest.mark.parametrize("case,offset_dtype", [(gc.cases(SMALL)["e"][1], np.int32), (gc.cases(SMALL)["i"][0], np.int64)],
                         ids=lambda p: repr(p) if isinstance(p, gc.Case) else np.dtype(p).name)
def test_exact_sweeps_and_launch_counts_over_every_knob(case, offset_dtype):
    kk, be = backend()
    gc.check_knob_sweep(kk, be, case, DTYPES, offset_dtype, tc.LANES, tc.CHAIN_ROWS, tc.CHAIN_LEVELS)


# 4 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", gc.all_cases(SMALL, ("c", "e", "g", "i")), ids=repr)
def test_composition_bit_for_bit(case):
    kk, be = backend()
    gc.check_composition(kk, be, case)


# 5 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", gc.all_cases(SMALL, ("c", "d", "e", "f", "g")), ids=repr)
def test_one_rounded_sweep_meets_the_local_bound(case):
    kk, be = backend()
    values, x0, y = case.rounded
    sm = gc.Smoother(kk, be, case)
    for dtype in DTYPES:
        for direction in gc.DIRECTIONS:
            x = sm.apply(direction, values, x0, y, dtype, omega=0.9)
            gc.local_bound_check(case, values.astype(dtype), x0.astype(dtype), y.astype(dtype), x, direction, dtype(0.9), dtype)
    sm.close()


# 6 and 7 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nv", [5, 17])
@pytest.mark.parametrize("layout", ["left", "right", "strided-left", "strided-right"])
def test_rank_2_columns_equal_rank_1(nv, layout):
    kk, be = backend()
    gc.check_rank2(kk, be, gc.cases(SMALL)["g"][1], nv, layout, np.float64 if nv == 5 else np.float32)


def test_ghost_entries_are_read_and_come_back_unchanged():
    kk, be = backend()
    gc.check_ghost_entries(kk, be, SMALL)


# 8 ----------------------------------------------------------------------------------------------------------------------------------

def test_symmetric_iterations_reduce_the_error():
    """the reference's own criterion (sparse/unit_test/Test_Sparse_gauss_seidel.hpp): with y = A x*, the error after symmetric
    iterations from x = 0 falls below the initial error, and further with more iterations"""
    kk, be = backend()
    gc.check_convergence(kk, be, gc.cases(SMALL)["c"][1])


# 9 ----------------------------------------------------------------------------------------------------------------------------------

def test_error_statuses():
    kk, be = backend()
    gc.check_statuses(kk, be, gc.cases(SMALL)["d"][0])


def test_empty_matrix():
    kk, be = backend()
    gc.check_empty(kk, be, SMALL)

