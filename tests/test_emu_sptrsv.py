"""Sparse triangular solve under the SIMT emulator: kk_sptrsv.hip compiled by g++ against kk_emu.h (tests/emu/sptrsv.mk, which includes
tests/emu/Makefile and adds the one unit) -- level sets against the restated reference loops, exact values over every knob, launch
counts, error statuses.  Cases are cut to emulator size (tests/sptrsv_cases.py, small=True)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np
import pytest

import kk_loader
import sptrsv_cases as sc
from emu import emu_backend

HERE = os.path.dirname(os.path.abspath(emu_backend.__file__))
SO = os.path.join(HERE, "libkkamd_emu_sptrsv.so")
_BACKEND = None


def backend():
    global _BACKEND
    if _BACKEND is None:
        kk = kk_loader.load()
        with open(emu_backend.LOCK, "w") as lk:           # the lock emu_backend.build() takes: the objects are shared
            fcntl.flock(lk, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-C", HERE, "-f", "sptrsv.mk", "-s", "libkkamd_emu_sptrsv.so"])
        lib = kk._capi.bind(C.CDLL(SO))
        _BACKEND = kk.Backend(lib, lambda n, dt: np.zeros(int(n), dtype=dt), lambda a: None if a is None else a.ctypes.data,
                              lambda: None, lambda a: a, lambda a: np.array(a, copy=True), "emu")
    return kk_loader.load(), _BACKEND


TRIANGLES = sc.all_triangles(True)


@pytest.mark.parametrize("offset_dtype", [np.int32, np.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("tri", TRIANGLES, ids=repr)
def test_level_sets_match_reference_loops(tri, offset_dtype):
    kk, be = backend()
    an = sc.Analysed(kk, be, tri, "SEQLVLSCHD_TP1", offset_dtype)
    sc.check_level_sets(an)
    # a second symbolic call on the same handle analyses again
    kk.sptrsv_symbolic(an.kh, an.row_map, an.entries)
    sc.check_level_sets(an)
    an.close()


@pytest.mark.parametrize("algo", ["SEQLVLSCHD_RP", "SEQLVLSCHD_TP1", "SEQLVLSCHD_TP1CHAIN"])
@pytest.mark.parametrize("tri", TRIANGLES, ids=repr)
def test_exact_values_default_knobs(tri, algo):
    kk, be = backend()
    for offset_dtype, dtype in ((np.int32, np.float64), (np.int64, np.float32)):
        an = sc.Analysed(kk, be, tri, algo, offset_dtype)
        sc.check_exact(an, dtype)
        sc.check_exact(an, dtype, alias=True)
        an.close()


# one form of every case: lower and upper, both orders of entries and both offset types between them
@pytest.mark.parametrize("tri,offset_dtype", [(v[(1, 2)[i % 2]], (np.int32, np.int64)[i % 2]) for i, v in enumerate(sc.cases(True).values())],
                         ids=lambda p: repr(p) if isinstance(p, sc.Triangle) else np.dtype(p).name)
def test_exact_values_and_launch_counts_over_every_knob(tri, offset_dtype):
    kk, be = backend()
    sc.check_knob_sweep(kk, be, tri, (np.float64, np.float32), offset_dtype)


def test_bidiagonal_is_one_chain_per_chain_levels():
    kk, be = backend()
    tri = sc.cases(True)["d"][0]
    an = sc.Analysed(kk, be, tri, "SEQLVLSCHD_TP1CHAIN")
    assert an.th.get_num_levels() == tri.n and an.th.get("max_level_rows") == 1
    assert an.th.get("chain_rows") == 64 and an.th.get("chain_levels") == 1024 and an.th.get("lanes_per_row") == 0
    assert (an.th.get("launches"), an.th.get("chain_launches"), an.th.get("chained_levels")) == (1, 1, tri.n)
    an.th.set("chain_levels", 16)
    assert an.th.get("launches") == -(-tri.n // 16)
    assert an.th.get("plan_bytes") == 12 * tri.n + 8 * (tri.n + 1)
    an.close()


@pytest.mark.parametrize("algo", ["SEQLVLSCHD_RP", "SEQLVLSCHD_TP1CHAIN"])
def test_empty_matrix(algo):
    """0 rows: an analysis with no level, no launch and nothing kept on the device; the solve returns"""
    kk, be = backend()
    kh = kk.KokkosKernelsHandle(be)
    kh.create_sptrsv_handle(algo, 0, True)
    th = kh.get_sptrsv_handle()
    row_map, entries = be.from_numpy(np.zeros(1, dtype=np.int32)), be.from_numpy(np.zeros(0, dtype=np.int32))
    kk.sptrsv_symbolic(kh, row_map, entries)
    assert th.is_symbolic_complete()
    assert {k: th.get(k) for k in ("num_levels", "launches", "max_level_rows", "plan_bytes")} == \
        {"num_levels": 0, "launches": 0, "max_level_rows": 0, "plan_bytes": 0}
    for what in ("level_list", "nodes_per_level", "nodes_grouped_by_level"):
        assert th.export(what).shape == (0,)
    th.set("chain_levels", 16)                               # plans again
    assert th.get("launches") == 0
    val, b, x = (be.from_numpy(np.zeros(0)) for _ in range(3))
    assert kk.sptrsv_solve(kh, row_map, entries, val, b, x) is x
    assert be.lib.kkamd_sptrsv_solve(th.h, 0, None, None, None, None, None, 0, 1, None) == kk._capi.OK
    kh.destroy_sptrsv_handle()


def _status(fn):
    kk = kk_loader.load()
    with pytest.raises(kk.KkamdError) as e:
        fn()
    return e.value.status, str(e.value)


def _lower3(be, entries, row_map=(0, 1, 3, 6)):
    return be.from_numpy(np.array(row_map, dtype=np.int32)), be.from_numpy(np.array(entries, dtype=np.int32))


def test_error_statuses():
    kk, be = backend()
    cap = kk._capi
    kh = kk.KokkosKernelsHandle(be)
    st, msg = _status(lambda: kh.create_sptrsv_handle("SPTRSV_CUSPARSE", 3, True))
    assert st == cap.ERR_UNSUPPORTED
    with pytest.raises(RuntimeError):
        kh.create_sptrsv_handle("SEQLVLSCHD_XX", 3, True)
    with pytest.raises(ValueError):                          # no SPTRSV handle on the KernelHandle
        kk.sptrsv_symbolic(kh, *_lower3(be, [0, 0, 1, 0, 1, 2]))
    kh.create_sptrsv_handle("SEQLVLSCHD_TP1", 3, True)
    th = kh.get_sptrsv_handle()
    good = _lower3(be, [0, 1, 0, 2, 0, 1])
    val = be.from_numpy(np.ones(6)); b = be.from_numpy(np.ones(3)); x = be.from_numpy(np.zeros(3))
    # solve before symbolic
    with pytest.raises(ValueError, match="symbolic"):
        kk.sptrsv_solve(kh, good[0], good[1], val, b, x)
    assert be.lib.kkamd_sptrsv_solve(th.h, 3, be.ptr(good[0]), be.ptr(good[1]), be.ptr(val), be.ptr(b), be.ptr(x), 0, 1, None) == cap.ERR_STATE
    # num_rows differs from the handle's
    rm4 = be.from_numpy(np.array([0, 1, 2, 3, 4], dtype=np.int32)); e4 = be.from_numpy(np.arange(4, dtype=np.int32))
    st, msg = _status(lambda: kk.sptrsv_symbolic(kh, rm4, e4))
    assert st == cap.ERR_INVALID_ARG and "differs" in msg
    # each structural fault names the first offending row (row 1 and row 2 are both faulty in every case)
    for entries, word in (([0, 1, 7, 2, -1, 0], "outside"), ([0, 2, 1, 2, 0, 2], "above"), ([0, 0, 0, 0, 1, 1], "no diagonal"),
                          ([0, 1, 1, 2, 2, 0], "more than one diagonal")):
        st, msg = _status(lambda: kk.sptrsv_symbolic(kh, *_lower3(be, entries)))
        assert st == cap.ERR_INVALID_ARG and "row 1:" in msg and word in msg, msg
        assert not th.is_symbolic_complete()
    khu = kk.KokkosKernelsHandle(be)
    khu.create_sptrsv_handle("SEQLVLSCHD_RP", 3, False)
    st, msg = _status(lambda: kk.sptrsv_symbolic(khu, *_lower3(be, [0, 1, 2, 1, 0, 2], (0, 3, 4, 6))))
    assert st == cap.ERR_INVALID_ARG and "row 2:" in msg and "below" in msg
    # a failed analysis leaves the handle without one; a good one completes it
    kk.sptrsv_symbolic(kh, *good)
    assert th.is_symbolic_complete() and th.get_num_levels() == 3
    # unsupported value type, knob ranges, unknown keys
    assert be.lib.kkamd_sptrsv_solve(th.h, 3, be.ptr(good[0]), be.ptr(good[1]), be.ptr(val), be.ptr(b), be.ptr(x), 0, 5, None) == cap.ERR_UNSUPPORTED
    for key, bad in (("lanes_per_row", 3), ("lanes_per_row", 128), ("lanes_per_row", -1), ("chain_rows", -1), ("chain_levels", 0), ("nonsense", 1)):
        st, msg = _status(lambda: th.set(key, bad))
        assert st == cap.ERR_INVALID_ARG
    st, msg = _status(lambda: th.get("nonsense"))
    assert st == cap.ERR_INVALID_ARG
    st, msg = _status(lambda: th.export("nonsense"))
    assert st == cap.ERR_INVALID_ARG
    out = np.zeros(2, dtype=np.int32)
    assert be.lib.kkamd_sptrsv_export(th.h, b"level_list", out.ctypes.data, 2) == cap.ERR_INVALID_ARG
    kh.destroy_sptrsv_handle(); khu.destroy_sptrsv_handle()
    assert kh.get_sptrsv_handle() is None
