"""ILU(k) under the SIMT emulator: kk_spiluk.hip (and kk_sptrsv.hip, whose level sets it takes) compiled by g++ against kk_emu.h
(tests/emu/spiluk.mk, which includes tests/emu/Makefile and adds the two units) -- the graphs of L and U and the level sets against the
restated reference loop, exact factors over every knob, launch counts, error statuses; and the host side of the symbolic phase as a
stand-alone program under the address and undefined-behaviour sanitizers.  Cases are cut to emulator size (tests/spiluk_cases.py,
small=True)."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np
import pytest

import kk_loader
import spiluk_cases as ic
from emu import emu_backend

HERE = os.path.dirname(os.path.abspath(emu_backend.__file__))
SO = os.path.join(HERE, "libkkamd_emu_spiluk.so")
_BACKEND = None


def _make(target):
    with open(emu_backend.LOCK, "w") as lk:               # the lock emu_backend.build() takes: the objects are shared
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-C", HERE, "-f", "spiluk.mk", "-s", target])


def backend():
    global _BACKEND
    if _BACKEND is None:
        kk = kk_loader.load()
        _make("libkkamd_emu_spiluk.so")
        lib = kk._capi.bind(C.CDLL(SO))
        _BACKEND = kk.Backend(lib, lambda n, dt: np.zeros(int(n), dtype=dt), lambda a: None if a is None else a.ctypes.data,
                              lambda: None, lambda a: a, lambda a: np.array(a, copy=True), "emu")
    return kk_loader.load(), _BACKEND


PATTERNS = ic.all_patterns(True)


@pytest.mark.parametrize("fill_lev", [0, 1, 2, 3])
@pytest.mark.parametrize("pat", PATTERNS, ids=repr)
def test_symbolic_matches_reference_loop(pat, fill_lev):
    kk, be = backend()
    for offset_dtype in (np.int32, np.int64):
        f = ic.Factored(kk, be, pat, fill_lev, offset_dtype, slack=(0, 3)[fill_lev % 2])
        ic.check_symbolic(f)
        f.close()


def test_second_symbolic_call_with_another_fill_level():
    kk, be = backend()
    pat = ic.cases(True)["e7"][1]
    f = ic.Factored(kk, be, pat, 2)                         # sized for k = 2: the smaller patterns fit
    ic.check_symbolic(f)
    for k in (0, 1, 2):
        f.L_entries[:] = -1; f.U_entries[:] = -1
        f.symbolic(k)
        ic.check_symbolic(f)
        if k == 0:
            ic.check_exact(f, np.float64)
    f.close()


@pytest.mark.parametrize("pat,fill_lev", ic.exact_cases(True), ids=lambda p: repr(p) if isinstance(p, ic.Pattern) else "k%d" % p)
def test_exact_factors_default_knobs(pat, fill_lev):
    kk, be = backend()
    for offset_dtype, dtype in ((np.int32, np.float64), (np.int64, np.float32)):
        f = ic.Factored(kk, be, pat, fill_lev, offset_dtype)
        ic.check_exact(f, dtype)
        f.close()


# one form of every pattern: both orders of entries and both offset types between them; b at k = 2, the others at k = 0
@pytest.mark.parametrize("pat,offset_dtype", [(v[i % 2], (np.int32, np.int64)[i % 2]) for i, v in enumerate(ic.cases(True).values())],
                         ids=lambda p: repr(p) if isinstance(p, ic.Pattern) else np.dtype(p).name)
def test_exact_factors_and_launch_counts_over_every_knob(pat, offset_dtype):
    kk, be = backend()
    ic.check_knob_sweep(kk, be, pat, 2 if pat.name == "b" else 0, (np.float64, np.float32), offset_dtype, alternate=pat.name in ("c", "e27"))


def test_case_shapes():
    """the small cases reach the paths they are meant for"""
    kk, be = backend()
    c = ic.cases(True)
    f = ic.Factored(kk, be, c["c"][0], 0)
    longest = int((np.diff(f.sym.L_row_map) + np.diff(f.sym.U_row_map)).max())
    assert longest > 64                                     # beyond one pass of 64 lanes
    assert f.ih.get("stage_entries_per_lane") * 8 < longest  # the sweep's lane counts up to 8 leave rows to global memory
    assert f.ih.get("lanes_in_use") == 32 and f.ih.get("lanes_per_row") == 0       # mean U row 24.75
    f.close()
    f = ic.Factored(kk, be, c["d"][0], 0)
    assert f.ih.get_num_levels() == 24 and f.ih.get("max_level_rows") == 1
    assert f.ih.get("chain_rows") == 64 and f.ih.get("chain_levels") == 1024
    assert (f.ih.get("launches"), f.ih.get("chain_launches"), f.ih.get("chained_levels")) == (1, 1, 24)
    f.ih.set("chain_levels", 16)
    assert f.ih.get("launches") == 2
    assert f.ih.get("plan_bytes") == 4 * 24 + 8 * 25
    f.close()
    f = ic.Factored(kk, be, c["a"][0], 0)
    assert f.ih.get_num_levels() == 1 and f.ih.get("max_level_rows") == 70 and f.ih.get("plan_bytes") == 4 * 70 + 16
    f.close()


@pytest.mark.parametrize("name,pat,values,fill_lev", ic.g_cases(), ids=[g[0] for g in ic.g_cases()])
def test_zero_pivots_become_1e6(name, pat, values, fill_lev):
    kk, be = backend()
    sym = pat.symbolic(fill_lev)
    for dtype in (np.float64, np.float32):
        L, U = ic.reference_numeric(pat.row_map, pat.entries, values, sym, dtype)
        f = ic.Factored(kk, be, pat, fill_lev)
        ic.check_symbolic(f)
        lv, uv = f.numeric(values, dtype)
        assert np.array_equal(lv, L) and np.array_equal(uv, U)
        diag = uv[sym.U_row_map[:-1]]
        if name == "g-missing":
            assert diag[2] == -6 and diag[4] == 1e6 and diag[5] == 1e6 and (diag[[0, 1, 3]] != 1e6).all()
        else:
            assert diag[1] == 1e6 and diag[0] == 1
        f.close()


def test_rounded_values_meet_the_identity_bound():
    """the restated recurrence and the kernels, both inside the bound of spiluk_cases.identity_check"""
    kk, be = backend()
    for name in ("b", "c", "e27", "e7"):
        pat = ic.cases(True)[name][1]
        for k in (0, 1, 2):
            sym = pat.symbolic(k)
            f = ic.Factored(kk, be, pat, k)
            for dtype in (np.float64, np.float32):
                A = pat.rounded.astype(dtype)
                ic.identity_check(pat, sym, A, *ic.reference_numeric(pat.row_map, pat.entries, A, sym, dtype), dtype)
                ic.identity_check(pat, sym, A, *f.numeric(A, dtype), dtype)
            f.close()


def test_empty_matrix():
    """0 rows: an analysis with no level and no launch, whose plan_bytes counts the one level offset; numeric returns"""
    kk, be = backend()
    kh = kk.KokkosKernelsHandle(be)
    kh.create_spiluk_handle("SEQLVLSCHD_TP1", 0, 0, 0)
    ih = kh.get_spiluk_handle()
    rm = lambda: be.from_numpy(np.zeros(1, dtype=np.int32))
    ent = lambda: be.from_numpy(np.zeros(0, dtype=np.int32))
    A_rm, A_ent, L_rm, L_ent, U_rm, U_ent = rm(), ent(), rm(), ent(), rm(), ent()
    kk.spiluk_symbolic(kh, 1, A_rm, A_ent, L_rm, L_ent, U_rm, U_ent)
    assert ih.is_symbolic_complete() and (ih.get_nnzL(), ih.get_nnzU()) == (0, 0)
    assert {k: ih.get(k) for k in ("num_levels", "launches", "max_level_rows", "plan_bytes")} == \
        {"num_levels": 0, "launches": 0, "max_level_rows": 0, "plan_bytes": 8}
    assert ih.export("level_list").shape == (0,) and ih.export("level_idx").shape == (0,)
    assert np.array_equal(ih.export("level_ptr"), [0])
    ih.set("chain_levels", 16)                              # plans again
    assert ih.get("launches") == 0
    val = lambda: be.from_numpy(np.zeros(0))
    kk.spiluk_numeric(kh, 1, A_rm, A_ent, val(), L_rm, L_ent, val(), U_rm, U_ent, val())
    assert be.lib.kkamd_spiluk_numeric(ih.h, 1, 0, *[None] * 9, 0, 1, None) == kk._capi.OK
    kh.destroy_spiluk_handle()


def _status(fn):
    kk = kk_loader.load()
    with pytest.raises(kk.KkamdError) as e:
        fn()
    return e.value.status, str(e.value)


def test_error_statuses():
    kk, be = backend()
    cap = kk._capi
    pat = ic.cases(True)["b"][0]
    sym = pat.symbolic(1)
    kh = kk.KokkosKernelsHandle(be)
    with pytest.raises(RuntimeError):
        kh.create_spiluk_handle("SEQLVLSCHED_TP2", pat.n, 1, 1)
    i32 = lambda a: be.from_numpy(np.array(a, dtype=np.int32))
    A_rm, A_ent = i32(pat.row_map), i32(pat.entries)
    L_rm, U_rm = i32(np.full(pat.n + 1, -1)), i32(np.full(pat.n + 1, -1))
    L_ent, U_ent = i32(np.full(sym.nnzL, -1)), i32(np.full(sym.nnzU, -1))
    with pytest.raises(ValueError):                          # no SPILUK handle on the KernelHandle
        kk.spiluk_symbolic(kh, 1, A_rm, A_ent, L_rm, L_ent, U_rm, U_ent)
    kh.create_spiluk_handle("SEQLVLSCHD_TP1", pat.n, sym.nnzL, sym.nnzU)
    ih = kh.get_spiluk_handle()
    val = be.from_numpy(np.ones(pat.entries.shape[0])); lv = be.from_numpy(np.zeros(sym.nnzL)); uv = be.from_numpy(np.zeros(sym.nnzU))
    numeric_args = (ih.h, 1, pat.n, be.ptr(A_rm), be.ptr(A_ent), be.ptr(val), be.ptr(L_rm), be.ptr(L_ent), be.ptr(lv), be.ptr(U_rm), be.ptr(U_ent),
                    be.ptr(uv), 0)
    # numeric before symbolic
    with pytest.raises(ValueError, match="symbolic"):
        kk.spiluk_numeric(kh, 1, A_rm, A_ent, val, L_rm, L_ent, lv, U_rm, U_ent, uv)
    assert be.lib.kkamd_spiluk_numeric(*numeric_args, 1, None) == cap.ERR_STATE
    st, msg = _status(lambda: ih.export("level_list"))
    assert st == cap.ERR_STATE
    # capacity one too small: the reference's words with the true count, and nothing written
    for which in ("L", "U"):
        small_L = i32(np.full(sym.nnzL - (which == "L"), -1)); small_U = i32(np.full(sym.nnzU - (which == "U"), -1))
        st, msg = _status(lambda: kk.spiluk_symbolic(kh, 1, A_rm, A_ent, L_rm, small_L, U_rm, small_U))
        need, have = (sym.nnzL, sym.nnzL - 1) if which == "L" else (sym.nnzU, sym.nnzU - 1)
        assert st == cap.ERR_INVALID_ARG and "%s_entries's extent must be larger than %d, must be at least %d" % (which, have, need) in msg, msg
        assert (small_L == -1).all() and (small_U == -1).all() and (L_rm == -1).all() and (U_rm == -1).all()
        assert not ih.is_symbolic_complete()
    # negative fill level: the reference's message
    st, msg = _status(lambda: kk.spiluk_symbolic(kh, -1, A_rm, A_ent, L_rm, L_ent, U_rm, U_ent))
    assert st == cap.ERR_INVALID_ARG and "fill_lev: -1. Valid value is >= 0." in msg
    # wrong num_rows
    st, msg = _status(lambda: kk.spiluk_symbolic(kh, 1, i32(pat.row_map[:-1]), A_ent, i32(np.zeros(pat.n)), L_ent, i32(np.zeros(pat.n)), U_ent))
    assert st == cap.ERR_INVALID_ARG and "differs" in msg
    # structural faults name the first offending row (row 1 and row 2 are faulty in every case)
    kh3 = kk.KokkosKernelsHandle(be)
    kh3.create_spiluk_handle("SEQLVLSCHD_TP1", 3, 9, 9)
    out = lambda: (i32(np.full(4, -1)), i32(np.full(9, -1)), i32(np.full(4, -1)), i32(np.full(9, -1)))
    for row_map, entries, word in (((0, 1, 4, 7), [0, 0, 1, 0, 2, 2, 1], "repeated"), ((0, 1, 3, 5), [0, 1, 3, 2, -1], "outside"),
                                   ((0, 2, 1, 3), [0, 1, 1], "not ascending")):
        st, msg = _status(lambda: kk.spiluk_symbolic(kh3, 1, i32(row_map), i32(entries), *out()))
        assert st == cap.ERR_INVALID_ARG and "row 1:" in msg and word in msg, msg
        assert not kh3.get_spiluk_handle().is_symbolic_complete()
    kh3.destroy_spiluk_handle()
    # a failed analysis leaves the handle without one; a good one completes it
    kk.spiluk_symbolic(kh, 1, A_rm, A_ent, L_rm, L_ent, U_rm, U_ent)
    assert ih.is_symbolic_complete() and (ih.get_nnzL(), ih.get_nnzU()) == (sym.nnzL, sym.nnzU)
    # unsupported value type, wrong num_rows at numeric, knob ranges, unknown keys
    assert be.lib.kkamd_spiluk_numeric(*numeric_args, 5, None) == cap.ERR_UNSUPPORTED
    assert be.lib.kkamd_spiluk_numeric(ih.h, 1, pat.n + 1, *numeric_args[3:], 1, None) == cap.ERR_INVALID_ARG
    for key, bad in (("lanes_per_row", 3), ("lanes_per_row", 128), ("lanes_per_row", -1), ("chain_rows", -1), ("chain_levels", 0), ("nonsense", 1)):
        st, msg = _status(lambda: ih.set(key, bad))
        assert st == cap.ERR_INVALID_ARG
    st, msg = _status(lambda: ih.get("nonsense"))
    assert st == cap.ERR_INVALID_ARG
    st, msg = _status(lambda: ih.export("nonsense"))
    assert st == cap.ERR_INVALID_ARG
    buf = np.zeros(2, dtype=np.int32)
    assert be.lib.kkamd_spiluk_export(ih.h, b"level_list", buf.ctypes.data, 2) == cap.ERR_INVALID_ARG
    h = C.c_void_p()
    assert be.lib.kkamd_spiluk_create(C.byref(h), 1, 3, 3, 3) == cap.ERR_INVALID_ARG      # SEQLVLSCHD_TP1 is the only algorithm
    assert be.lib.kkamd_spiluk_create(C.byref(h), 0, -1, 3, 3) == cap.ERR_INVALID_ARG
    kh.destroy_spiluk_handle()
    assert kh.get_spiluk_handle() is None


def test_host_fill_loop_under_the_sanitizers():
    """kk_spiluk_fill.h indexes by caller data: its validation and fill loop as a stand-alone program built with
    -fsanitize=address,undefined, fed malformed and good graphs (tests/emu/spiluk_fill_check.cpp)"""
    _make("spiluk_fill_check")
    r = subprocess.run([os.path.join(HERE, "spiluk_fill_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all passed" in r.stdout, r.stdout + r.stderr
