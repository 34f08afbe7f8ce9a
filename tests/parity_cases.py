"""Parity checks shared by the emulator tests (CPU, small sizes) and the GPU tests (`-m gpu`, through
the C ABI of libkkamd.so).  Every check compares the library under test with the CPU oracle on the same
seeded inputs, with the reference's own comparators and tolerances:
  SpMV   |expected - y| <= 10*eps*(beta*max_y + alpha*max_row*max_val*max_x), NaN mismatch fails
         (sparse/unit_test/Test_Sparse_spmv.hpp:84-91,181,432)
  SpGEMM row_map and entries IDENTICAL, values |a-b|/(|a|+|b|) <= 1e-7
         (sparse/unit_test/Test_Sparse_Utils.hpp:39-127)
"""
import math
import re

import numpy as np

import kk_loader
import oracle

kk = kk_loader.load()
EPS_F = float(np.finfo(np.float32).eps)


def dev(be, A0, offset_dtype=np.int32, value_dtype=None):
    vals = A0.values if value_dtype is None else A0.values.astype(value_dtype)
    return kk.CrsMatrix.from_host(A0.nrows, A0.ncols, A0.row_map, A0.entries, vals, offset_dtype=offset_dtype, backend=be)


def fspmv_ok(expected, got, tol):
    nan_mismatch = np.isnan(expected) ^ np.isnan(got)
    err = np.abs(expected - got)
    bad = nan_mismatch | (err > tol)
    return not bad.any(), (float(np.nanmax(err)) if err.size else 0.0)


# ------------------------------------------------------------------------------------------- views of padded parents
# A vector or multivector under test can be a window of a larger parent: every parent cell outside the window holds NaN (X) or a
# fixed sentinel bit pattern (Y) before the call and must hold the same bits after it.  A read outside the window then reaches a NaN
# (a NaN mismatch inside the window), a write outside it breaks the sentinel.  The parents are padded on all four sides, so a wrong
# access lands in memory the test owns.
SENTINEL_BITS = {np.dtype(np.float64): np.uint64(0x7FF8C0DE5EA1F00D), np.dtype(np.float32): np.uint32(0x7FC5EA1D)}
_UINT = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}
VIEWS = ("even_pitch", "odd_start", "tall")


def view_spec(kind, nvec, itemsize):
    """(left, right, top, bottom) padding of the parent around an n x nvec window:
      even_pitch  a row-major parent's pitch is even and the window's base 16-byte aligned: an odd width reaches the paired
                  16-byte stores next to the masked last column
      odd_start   the window begins at an odd column: a row-major base 8 (fp64) / 4 (fp32) bytes off 16-byte alignment, even pitch
      tall        an odd number of extra rows above and more below: a column-major parent's ld exceeds the window's rows and its
                  first row is odd"""
    if kind == "even_pitch":
        left = 16 // itemsize
        return (left, 1 if (left + nvec) % 2 else 2, 2, 1)
    if kind == "odd_start":
        return (1, 1 if nvec % 2 == 0 else 2, 2, 3)
    if kind == "tall":
        return (1, 1, 1, 2)
    return tuple(kind)


def _window_2d(be, M, order, pad, fill_bits=None):
    """M as the window of a padded parent in `order`; cells outside hold NaN, or the bit pattern fill_bits.  Returns (device window,
    device parent, host copy of the parent, window slices)"""
    left, right, top, bottom = pad
    n, k = M.shape
    P = np.empty((top + n + bottom, left + k + right), dtype=M.dtype, order=order)
    if fill_bits is None:
        P[...] = np.nan
    else:
        P.view(_UINT[P.dtype])[...] = fill_bits
    win = (slice(top, top + n), slice(left, left + k))
    P[win] = M
    Pd = _to_dev_2d(be, P)
    return Pd[win], Pd, P.copy(order="K"), win


def _window_1d(be, v, stride, pad=3, fill_bits=None):
    """v as every stride-th element of a parent padded by `pad` elements at both ends (NaN or fill_bits elsewhere)"""
    P = np.empty(2 * pad + max(v.size, 1) * stride, dtype=v.dtype)
    if fill_bits is None:
        P[...] = np.nan
    else:
        P.view(_UINT[P.dtype])[...] = fill_bits
    win = slice(pad, pad + v.size * stride, stride)
    P[win] = v
    Pd = be.from_numpy(P)
    return Pd[win], Pd, P.copy(), win


def assert_outside_unchanged(before, after, win, what):
    """every cell of the parent outside the window bit-identical to what it held before the call"""
    outside = np.ones(before.shape, dtype=bool)
    outside[win] = False
    u = _UINT[before.dtype]
    bad = (before.view(u) != after.view(u)) & outside
    if bad.any():
        at = np.argwhere(bad)[0]
        raise AssertionError("sentinel overwritten outside the %s view: %d cells, first at parent %s (window %s): %r" %
                             (what, int(bad.sum()), tuple(int(i) for i in at), win, after[tuple(at)]))


def check_spmv(be, A0, mode="N", alpha=1.0, beta=0.0, algo=None, nans=False, seed=0, offset_dtype=np.int32,
               max_val=1.0, knobs=None, value_dtype=None, vec_dtype=np.float64, expect=None, x_stride=1, y_stride=1):
    """one check_spmv() of the reference test (Test_Sparse_spmv.hpp:168-216).  x_stride / y_stride != 1: x and y are strided views
    of padded parents (NaN around x, a sentinel around y) whose cells outside the view must come back bit-identical"""
    rng = np.random.default_rng(seed)
    trans = mode in "TH"
    nin, nout = (A0.nrows, A0.ncols) if trans else (A0.ncols, A0.nrows)
    x = rng.random(nin).astype(vec_dtype)
    y0 = rng.random(nout).astype(vec_dtype)
    if nans:
        y0[::19] = np.nan
    A = dev(be, A0, offset_dtype, value_dtype)
    views = x_stride != 1 or y_stride != 1
    if views:
        xd, xpd, xp0, xwin = _window_1d(be, x, x_stride)
        yd, ypd, yp0, ywin = _window_1d(be, y0, y_stride, fill_bits=SENTINEL_BITS[np.dtype(vec_dtype)])
    else:
        xd, yd = be.from_numpy(x), be.from_numpy(y0)
    h = None
    if algo is None:
        kk.spmv(mode, alpha, A, xd, beta, yd)
    else:
        h = kk.SPMVHandle(algo)
        for k_, v_ in (knobs or {}).items():
            h.set(k_, v_)
        kk.spmv(h, mode, alpha, A, xd, beta, yd)
        kk.spmv(h, mode, alpha, A, xd, beta, yd) if beta == 0.0 else None   # handle reuse
        for k_, v_ in (expect or {}).items():                               # what the analysis must have produced
            assert h.query(k_) == v_, "plan query %s: %r, expected %r" % (k_, h.query(k_), v_)
    if views:
        yp = be.to_numpy(ypd)
        assert_outside_unchanged(yp0, yp, ywin, "y")
        assert_outside_unchanged(xp0, be.to_numpy(xpd), slice(0, 0), "x")       # x is never written, inside the view or out
        got = yp[ywin].astype(np.float64)
    else:
        got = be.to_numpy(yd).astype(np.float64)
    Ao = A0 if value_dtype is None else oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, A0.values.astype(value_dtype))
    if vec_dtype == np.float64:
        exp = oracle.spmv_serial(mode, Ao, alpha, x, beta, y0.copy())
        eps_scale = 1.0
    else:
        exp = oracle.spmv_serial(mode, Ao, alpha, x, beta, y0.copy()).astype(np.float64)
        eps_scale = EPS_F / np.finfo(np.float64).eps
    tol = oracle.spmv_max_error(A0, alpha, beta, max_val=max_val) * eps_scale
    if trans and A0.nnz:      # a transposed product accumulates per COLUMN: scale the reference's bound by the longest column instead
        longest_col = int(np.bincount(A0.entries, minlength=A0.ncols).max()); longest_row = int(np.diff(A0.row_map).max())
        tol *= max(1.0, longest_col / max(longest_row, 1))
    ok, err = fspmv_ok(exp, got, max(tol, 1e-300))
    assert ok, "spmv mismatch mode=%s alpha=%g beta=%g algo=%s strides=%d,%d: max err %g > tol %g" % (mode, alpha, beta, algo, x_stride, y_stride, err, tol)
    return h


def check_spmv_mv(be, A0, nvec, mode="N", alpha=1.0, beta=0.0, x_order="F", y_order="F", algo=None, seed=0, knobs=None, expect=None,
                  max_val=1.0, nans=False, offset_dtype=np.int32, value_dtype=None, x_special=None, vec_dtype=np.float64, view=None):
    """x_special: {row: value} written into every column of X after the random fill (Inf / NaN propagation).
    vec_dtype: the scalar type of X and Y (fp32 vectors need value_dtype=np.float32).  view: X and Y are windows of padded parents
    in x_order / y_order (a name of VIEWS or a (left, right, top, bottom) tuple): NaN around X, a sentinel around Y, every cell outside
    the windows bit-identical after the call"""
    rng = np.random.default_rng(seed)
    trans = mode in "TH"
    vdt = np.dtype(vec_dtype)
    nin, nout = (A0.nrows, A0.ncols) if trans else (A0.ncols, A0.nrows)
    X = np.asarray(rng.random((nin, nvec)), order=x_order).astype(vdt, order="K")
    for r_, v_ in (x_special or {}).items():
        X[r_, :] = v_
    Y0 = np.asarray(rng.random((nout, nvec)), order=y_order).astype(vdt, order="K")
    if nans:
        Y0[::7, :] = np.nan
    if value_dtype is not None:
        A0 = oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, A0.values.astype(value_dtype).astype(np.float64))
    A = dev(be, A0, offset_dtype, value_dtype)
    if view is not None:
        Xd, Xpd, Xp0, xwin = _window_2d(be, X, x_order, view_spec(view, nvec, vdt.itemsize))
        Yd, Ypd, Yp0, ywin = _window_2d(be, Y0, y_order, view_spec(view, nvec, vdt.itemsize), fill_bits=SENTINEL_BITS[vdt])
    else:
        Xd, Yd = _to_dev_2d(be, X), _to_dev_2d(be, Y0)
    h = None
    if algo is None:
        kk.spmv(mode, alpha, A, Xd, beta, Yd)
    else:
        h = kk.SPMVHandle(algo)
        for k_, v_ in (knobs or {}).items():
            h.set(k_, v_)
        kk.spmv(h, mode, alpha, A, Xd, beta, Yd)
        if beta == 0.0:
            kk.spmv(h, mode, alpha, A, Xd, beta, Yd)                            # handle reuse
        for k_, v_ in (expect or {}).items():
            assert h.query(k_) == v_, "plan query %s: %r, expected %r" % (k_, h.query(k_), v_)
    if view is not None:
        Yp = _to_host_2d(be, Ypd)
        assert_outside_unchanged(Yp0, Yp, ywin, "Y")
        assert_outside_unchanged(Xp0, _to_host_2d(be, Xpd), (slice(0, 0), slice(0, 0)), "X")
        got = Yp[ywin].astype(np.float64)
    else:
        got = _to_host_2d(be, Yd).astype(np.float64)
    # the expected result in float64 from the (fp32-rounded) inputs; fp32 vectors scale the reference's bound by EPS_F / eps(f64)
    exp = oracle.spmv_mv_serial(mode, A0, alpha, X.astype(np.float64, order="K"), beta, Y0.astype(np.float64, order="K"))
    tol = oracle.spmv_max_error(A0, alpha, beta, max_val=max_val)
    if vdt == np.float32:
        tol *= EPS_F / np.finfo(np.float64).eps
    if trans and A0.nnz:      # a transposed product accumulates per COLUMN: scale the reference's bound by the longest column instead (as check_spmv does)
        longest_col = int(np.bincount(A0.entries, minlength=A0.ncols).max()); longest_row = int(np.diff(A0.row_map).max())
        tol *= max(1.0, longest_col / max(longest_row, 1))
    assert not (np.isnan(exp) ^ np.isnan(got)).any(), "spmv_mv NaN mismatch nvec=%d view=%s" % (nvec, view)
    inf = np.isinf(exp)
    assert np.array_equal(inf, np.isinf(got)) and np.array_equal(exp[inf], got[inf]), "spmv_mv Inf mismatch nvec=%d" % nvec
    exp = np.where(inf, 0.0, exp); got = np.where(inf, 0.0, got)
    err = np.nanmax(np.abs(exp - got)) if got.size else 0.0
    assert err <= max(tol, 1e-300), "spmv_mv mismatch nvec=%d mode=%s orders=%s%s view=%s %s: %g > %g" % (nvec, mode, x_order, y_order, view, vdt, err, tol)
    return h


def check_mv5(be, light=False):
    combos = ((16, "C", "C", 1.5, 0.5, np.int32), (16, "F", "F", 1.0, 0.0, np.int64), (5, "C", "F", 2.0, 0.0, np.int32), (37, "F", "C", -1.0, 1.0, np.int32),
              (32, "C", "C", 1.0, 0.0, np.int32))
    for ci, (name, A0, tiles, other) in enumerate(mv5_cases()):
        for nvec, xo, yo, alpha, beta, off in (combos if (ci < 3 or not light) else combos[:2]):
            h = check_spmv_mv(be, A0, nvec, "N", alpha, beta, xo, yo, algo="SPMV_DEFAULT", max_val=1.5, nans=(beta == 0.0), offset_dtype=off)
            got = h.query("mv5_tiles")
            assert (got > 0) if tiles is None else (got == tiles), (name, nvec, got, tiles)
            if other is not None and got > 0:
                assert h.query("mv5_other_rows") == other, (name, h.query("mv5_other_rows"))
    name, A0, _, _ = mv5_cases()[0]
    h = check_spmv_mv(be, A0, 16, "N", 1.0, 0.5, "C", "C", algo="SPMV_DEFAULT", max_val=1.5, value_dtype=np.float32)
    assert h.query("mv5_tiles") > 0 and h.query("mv5_fill_permille") == 1000
    # Inf / NaN in X: the rows that hold the column get it, the other rows of the tile do not (block 0: rows 0..31 hold column 3;
    # the band matrix: rows 90..110 hold column 100)
    for yo in ("C", "F"):
        h = check_spmv_mv(be, A0, 16, "N", 1.0, 0.0, "C", yo, algo="SPMV_DEFAULT", max_val=1.5, nans=True, x_special={3: np.inf, 40: np.nan, 1279: -np.inf})
        assert h.query("mv5_tiles") > 0
        h = check_spmv_mv(be, mv5_cases()[3][1], 7, "N", 1.0, 0.0, "F", yo, algo="SPMV_DEFAULT", max_val=1.5, nans=True, x_special={100: np.inf, 499: np.nan})
        assert h.query("mv5_tiles") > 0
    # forced (mv5 = 2: no fill threshold) on matrices it would not take, off (mv5 = 0), the gather kernel asked for, no analysis
    sparse = oracle.random_crs(800, 800, 9, variance=3, seed=5, sorted_rows=True)
    h = check_spmv_mv(be, sparse, 16, "N", 1.5, 0.0, "C", "C", algo="SPMV_DEFAULT", max_val=1.5, nans=True, knobs={"mv5": 2})
    assert h.query("mv5_tiles") > 10 and h.query("mv5_fill_permille") < 100, (h.query("mv5_tiles"), h.query("mv5_fill_permille"))
    h = check_spmv_mv(be, oracle.laplace2d("FE", 130, 41), 21, "N", 1.0, 1.0, "F", "F", algo="SPMV_DEFAULT", max_val=32.0, knobs={"mv5": 2})
    assert h.query("mv5_tiles") > 0
    # tiles whose union takes several chunks of 64 column blocks: 16 rows x 100 entries, no column shared (400 blocks per tile)
    wide = oracle.random_crs(48, 200000, 100, variance=0, seed=9, sorted_rows=True)
    for nvec, yo in ((16, "C"), (32, "F")):
        h = check_spmv_mv(be, wide, nvec, "N", 1.5, 0.0, "C", yo, algo="SPMV_DEFAULT", max_val=1.5, nans=True, knobs={"mv5": 2})
        assert h.query("mv5_tiles") >= 2 and h.query("mv5_blocks") > 2 * 300, (h.query("mv5_tiles"), h.query("mv5_blocks"))
    for algo, knobs in (("SPMV_DEFAULT", {"mv5": 0}), ("SPMV_DEFAULT", {"mv_kernel": 2}), ("SPMV_FAST_SETUP", None)):
        h = check_spmv_mv(be, A0, 16, "N", 1.0, 0.0, "C", "C", algo=algo, knobs=knobs, max_val=1.5)
        assert h.query("mv5_tiles") == 0


def mv6_cases():
    """(name, matrix) for the nonzero-split rank-2 kernel: chunks of 128 entries; rows cut by one and by many chunk boundaries, runs
    that end exactly at a boundary, empty rows (leading, trailing, in between), fewer entries than a chunk, one row only"""
    out = [("hubs", hub_matrix(3000, 9000, 6, {5: 7000, 17: 1500, 1234: 1025, 2999: 4000, 40: 1024}, seed=3))]
    rng = np.random.default_rng(31)
    def from_lens(lens, ncols, seed):
        lens = np.asarray(lens, dtype=np.int64)
        rm = np.zeros(lens.size + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
        r_ = np.random.default_rng(seed)
        ent = np.concatenate([np.sort(r_.choice(ncols, size=int(l), replace=False)) for l in lens] + [np.empty(0, np.int64)]).astype(np.int32)
        return oracle.Crs(lens.size, ncols, rm, ent, r_.random(int(rm[-1])) + 0.5)
    # every row exactly one chunk; rows of 64 (two per chunk); 128 + 1 (every boundary cuts a row one entry in)
    out.append(("rows of 128", from_lens([128] * 40, 4000, 1)))
    out.append(("rows of 64", from_lens([64] * 50, 4000, 2)))
    out.append(("rows of 129", from_lens([129] * 33, 4000, 3)))
    # empty rows everywhere, a row of 1000 in the middle, short rows
    lens = rng.integers(0, 9, 600); lens[:5] = 0; lens[-7:] = 0; lens[100:140] = 0; lens[300] = 1000; lens[301] = 0; lens[302] = 300
    out.append(("empty rows + long", from_lens(lens, 5000, 4)))
    out.append(("tiny", from_lens([3, 0, 5, 1], 50, 5)))
    out.append(("one row", from_lens([700], 2000, 6)))
    return out


def check_mv6(be, light=False):
    combos = ((16, "C", "C", 1.5, 0.5, np.int32), (16, "F", "F", 1.0, 0.0, np.int64), (5, "C", "F", 2.0, 0.0, np.int32), (33, "F", "C", -1.0, 1.0, np.int32))
    for ci, (name, A0) in enumerate(mv6_cases()):
        for nvec, xo, yo, alpha, beta, off in (combos if (ci < 2 or not light) else combos[:2]):
            h = check_spmv_mv(be, A0, nvec, "N", alpha, beta, xo, yo, algo="SPMV_DEFAULT", max_val=50.0, nans=(beta == 0.0), offset_dtype=off, knobs={"mv6": 2})
            assert h.query("mv6_chunks") == -(-A0.nnz // 128), (name, h.query("mv6_chunks"))
            assert h.query("mv6_empty_rows") == int((np.diff(A0.row_map) == 0).sum()), name
    name, A0 = mv6_cases()[0]
    # by default on matrices with a tenth of their entries in long rows; fp32 values; Inf / NaN in X
    h = check_spmv_mv(be, A0, 16, "N", 1.0, 0.5, "C", "C", algo="SPMV_DEFAULT", max_val=50.0, value_dtype=np.float32)
    assert h.query("mv6_chunks") > 0 and h.query("mv_long_nnz") == 7000 + 1500 + 1025 + 4000 + 1024
    h = check_spmv_mv(be, A0, 16, "N", 1.0, 0.0, "C", "C", algo="SPMV_DEFAULT", max_val=50.0, nans=True, x_special={int(A0.entries[0]): np.inf, 40: np.nan, 8999: -np.inf})
    assert h.query("mv6_chunks") > 0
    # not its matrices / off / the gather kernel asked for / no analysis
    h = check_spmv_mv(be, randomized(oracle.random_crs(2000, 2000, 9, variance=3, seed=5)), 16, "N", 1.0, 0.0, "C", "C", algo="SPMV_DEFAULT")
    assert h.query("mv6_chunks") == 0
    for algo, knobs in (("SPMV_DEFAULT", {"mv6": 0}), ("SPMV_DEFAULT", {"mv_kernel": 2}), ("SPMV_FAST_SETUP", None)):
        h = check_spmv_mv(be, A0, 16, "N", 1.0, 0.0, "C", "C", algo=algo, knobs=knobs, max_val=50.0)
        assert h.query("mv6_chunks") == 0


def check_transpose_plan_inherits_knobs(be):
    """Modes T / H of an analysed handle run the mode-N dispatch on the plan of its cached transpose: what the caller set on the handle --
    a forced rank-2 kernel, the nonzero-split kernel switched off -- must hold there too, whether it was set before the transpose exists
    (replayed at its creation) or afterwards (forwarded); round-4 advisor finding."""
    lib = be.lib
    kk._capi.check(lib, lib.kkamd_set_default(b"explicit_transpose_min_knnz", 0))
    try:
        name, A0 = mv6_cases()[0]
        At0 = oracle.transpose(A0)
        # the transpose of this matrix is one the nonzero-split kernel takes by default ...
        h = check_spmv_mv(be, A0, 16, "T", 1.0, 0.0, "C", "C", algo="SPMV_DEFAULT", max_val=50.0, knobs={"mv6": 2})
        assert h.query("transpose_plan_mv6_chunks") == -(-At0.nnz // 128), h.query("transpose_plan_mv6_chunks")
        # ... a handle with the gather kernel forced BEFORE the first transposed call keeps it away from the transpose's plan ...
        h = check_spmv_mv(be, A0, 16, "T", 1.0, 0.5, "C", "C", algo="SPMV_DEFAULT", max_val=50.0, knobs={"mv6": 2, "mv_kernel": 2})
        assert h.query("transpose_plan_tile") > 0 and h.query("transpose_plan_mv6_chunks") == 0
        # ... and setting it AFTERWARDS reaches the existing transposed plan
        h = check_spmv_mv(be, A0, 16, "T", 1.0, 0.0, "C", "C", algo="SPMV_DEFAULT", max_val=50.0, knobs={"mv6": 2})
        assert h.query("transpose_plan_mv6_chunks") > 0
        h.set("mv6", 0)
        assert h.query("transpose_plan_mv6_chunks") == 0
        assert h.query("transpose_bytes") >= At0.nnz * (4 + 4 + 8 + 8)          # structure, permutation, values and the shadow copy of exact tracking
    finally:
        kk._capi.check(lib, lib.kkamd_set_default(b"explicit_transpose_min_knnz", 1000))


def check_rank2_first_handle_defers_rank1(be):
    """A handle whose first call is rank 2 (more than one column) leaves the rank-1 analysis -- tiles, window codes, pattern records -- to
    the first rank-1 call (knob defer_rank1, set by SPMVHandle; the reference's handle is set up by its first call, for that call's rank,
    KokkosSparse_spmv_handle.hpp:280-349): rank 2, rank 1, rank 2 again on one handle, modes N and T, each against the oracle; the rank-1
    plan does not exist before the rank-1 call and does afterwards; a handle that begins with rank 1 is analysed at once, as before; the
    knob can be switched off on the handle."""
    lib = be.lib
    kk._capi.check(lib, lib.kkamd_set_default(b"explicit_transpose_min_knnz", 0))
    try:
        for A0 in (oracle.laplace3d("FE", 9, 8, 7), oracle.random_crs(900, 700, 14, variance=6, seed=21)):
            A = dev(be, A0)
            rng = np.random.default_rng(5)
            for mode in ("N", "T"):
                trans = mode == "T"
                nin, nout = (A0.nrows, A0.ncols) if trans else (A0.ncols, A0.nrows)
                X = np.asarray(rng.random((nin, 6)), order="C"); Y0 = np.asarray(rng.random((nout, 6)), order="C")
                x = rng.random(nin); y0 = rng.random(nout)
                tol2 = oracle.spmv_max_error(A0, 1.5, 0.5) * (max(1.0, np.bincount(A0.entries, minlength=A0.ncols).max() / max(np.diff(A0.row_map).max(), 1)) if trans else 1.0)
                h = kk.SPMVHandle("SPMV_DEFAULT")
                key = "transpose_plan_tiles" if trans else "tiles"
                def rank2():
                    Yd = _to_dev_2d(be, Y0)
                    kk.spmv(h, mode, 1.5, A, _to_dev_2d(be, X), 0.5, Yd)
                    exp = oracle.spmv_mv_serial(mode, A0, 1.5, X, 0.5, Y0.copy(order="K"))
                    assert np.abs(_to_host_2d(be, Yd) - exp).max() <= tol2, (mode, "rank 2")
                def rank1():
                    yd = be.from_numpy(y0)
                    kk.spmv(h, mode, 1.5, A, be.from_numpy(x), 0.5, yd)
                    exp = oracle.spmv_serial(mode, A0, 1.5, x, 0.5, y0.copy())
                    assert np.abs(be.to_numpy(yd) - exp).max() <= tol2, (mode, "rank 1")
                rank2()
                assert h.query("tile") > 0 and h.query("tiles") == 0, (h.query("tile"), h.query("tiles"))      # analysed handle, no rank-1 plan yet
                if trans: assert h.query("transpose_plan_tile") > 0 and h.query(key) == 0
                rank1()
                assert h.query(key) > 0, (mode, h.query(key))
                rank2(); rank1()
                # rank 1 first: analysed at creation
                h = kk.SPMVHandle("SPMV_DEFAULT")
                rank1()
                assert h.query(key) > 0
                rank2()
                # the knob switched off by the caller
                h = kk.SPMVHandle("SPMV_DEFAULT"); h.set("defer_rank1", 0)
                rank2()
                assert h.query("tiles") > 0
    finally:
        kk._capi.check(lib, lib.kkamd_set_default(b"explicit_transpose_min_knnz", 1000))


def check_colslab_deterministic(be):
    """The DETERMINISTIC column-slab form of rank-1 mode N (round 5; `colslab` 4 forces it, 3 -- the default -- chooses it by rule): per-slab
    partial sums of every row, stored by exactly one writer, cut runs summed in chunk order, slabs added in ascending order -- no atomics.
    Cases: rows longer than a wave's chunk of 512 entries inside ONE slab (runs cut by several chunk boundaries: head / tail / whole-chunk
    pieces), empty rows, rows with one entry per slab, duplicate columns, a matrix wider than tall, the last chunk shorter than a round,
    beta != 0, NaN in y with beta = 0, fp32 values / vectors, 64-bit offsets, value changes under exact tracking -- and the SAME BITS
    from two handles and from repeated calls."""
    import struct
    rng = np.random.default_rng(4)
    n, k = 1200, 5000
    lens = rng.integers(0, 12, size=n); lens[3] = 1700; lens[4] = 0; lens[5] = 3000; lens[700] = 4999; lens[n - 1] = 530
    rm = np.zeros(n + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
    ent = np.concatenate([np.sort(rng.choice(k, size=l, replace=False)) for l in lens]).astype(np.int32)
    ent[rm[5]:rm[5] + 2000] = np.sort(rng.integers(0, 60, size=2000))                 # 2000 entries (duplicates) of one row inside the first slab: a run over four chunks
    A0 = oracle.Crs(n, k, rm, ent, 1 + 49 * rng.random(rm[-1]))
    wide = oracle.random_crs(300, 9000, 40, variance=10, seed=6)
    for M in (A0, wide):
        for shift in (6, 9, 13):
            kn = {"colslab": 4, "colslab_shift": shift}
            h = check_spmv(be, M, "N", 1.5, 0.5, "SPMV_DEFAULT", knobs=kn, max_val=50.0, expect={"colslab": 1, "colslab_deterministic": 1})
            assert h.query("colslab_slabs") <= 64
            check_spmv(be, M, "N", 1.0, 0.0, "SPMV_DEFAULT", knobs=kn, max_val=50.0, nans=True)
        check_spmv(be, M, "N", -1.0, 2.0, "SPMV_DEFAULT", knobs={"colslab": 4, "colslab_shift": 7}, max_val=50.0, offset_dtype=np.int64, value_dtype=np.float32)
        check_spmv(be, M, "N", 1.0, 1.0, "SPMV_DEFAULT", knobs={"colslab": 4, "colslab_shift": 7, "colslab_const": 1}, max_val=50.0, value_dtype=np.float32, vec_dtype=np.float32)
    # the same bits: two handles, repeated calls, after a value change and back
    A = dev(be, A0)
    x = rng.random(k); xd = be.from_numpy(x)
    outs = []
    for rep in range(2):
        h = kk.SPMVHandle("SPMV_DEFAULT"); h.set("colslab", 4); h.set("colslab_shift", 6)
        yd = be.from_numpy(np.zeros(n))
        for call in range(2):
            kk.spmv(h, "N", 1.0, A, xd, 0.0, yd)
            outs.append(be.to_numpy(yd).copy())
        assert h.query("colslab_deterministic") == 1
    for o in outs[1:]:
        assert o.tobytes() == outs[0].tobytes(), "the deterministic column-slab form gave different bits"
    exp = oracle.spmv_serial("N", A0, 1.0, x, 0.0, np.zeros(n))
    np.testing.assert_allclose(outs[0], exp, rtol=1e-11, atol=1e-9)
    v = A0.values.copy(); v[::7] *= -2.0
    A.values[:] = be.from_numpy(v)                                # exact tracking (default): the copy follows
    kk.spmv(h, "N", 1.0, A, xd, 0.0, yd)
    exp2 = oracle.spmv_serial("N", oracle.Crs(n, k, rm, ent, v), 1.0, x, 0.0, np.zeros(n))
    np.testing.assert_allclose(be.to_numpy(yd), exp2, rtol=1e-11, atol=1e-9)
    # one handle, BOTH vector types (round-5 advice: the partial-sum buffers were sized by the first call's type and the other type got
    # KKAMD_ERR_STATE; the CRS kernels take either on one handle): a float matrix with fp64 vectors, then fp32 vectors, then fp64 again
    v32 = v.astype(np.float32)
    A32 = dev(be, oracle.Crs(n, k, rm, ent, v32.astype(np.float64)), value_dtype=np.float32)
    h32 = kk.SPMVHandle("SPMV_DEFAULT"); h32.set("colslab", 4); h32.set("colslab_shift", 6)
    exp64 = oracle.spmv_serial("N", oracle.Crs(n, k, rm, ent, v32.astype(np.float64)), 1.0, x, 0.0, np.zeros(n))
    x32 = x.astype(np.float32)
    exp32 = oracle.spmv_serial("N", oracle.Crs(n, k, rm, ent, v32.astype(np.float64)), 1.0, x32.astype(np.float64), 0.0, np.zeros(n))
    for vec32 in (False, True, False):
        if vec32:
            y32 = be.from_numpy(np.zeros(n, dtype=np.float32))
            kk.spmv(h32, "N", 1.0, A32, be.from_numpy(x32), 0.0, y32)
            np.testing.assert_allclose(be.to_numpy(y32).astype(np.float64), exp32, rtol=2e-4, atol=1e-2)
        else:
            kk.spmv(h32, "N", 1.0, A32, xd, 0.0, yd)
            np.testing.assert_allclose(be.to_numpy(yd), exp64, rtol=1e-11, atol=1e-9)
        assert h32.query("colslab_deterministic") == 1
    # the rule of the default handle says no on a small matrix (x is not several L2s large): nothing is built
    check_spmv(be, A0, "N", 1.0, 0.0, "SPMV_DEFAULT", max_val=50.0, expect={"colslab": 0, "colslab_tried": 1})


def check_values_tracking(be):
    """The re-ordered value copies of a plan (cached transpose, column-slab copy) under the three "values_tracking" policies: 0 exact
    (default), 1 notify (SPMVHandle.values_changed), 2 fingerprints.  A.values is rewritten in place between calls: one value, every value,
    two values swapped, a whole 4096-value tile negated and another doubled (the changes the round-3 linear fingerprint was blind or
    nearly blind to), then nothing."""
    lib = be.lib
    kk._capi.check(lib, lib.kkamd_set_default(b"explicit_transpose_min_knnz", 0))
    try:
        A0 = oracle.random_crs(2500, 2300, 10, variance=3, seed=8, sorted_rows=True)
        rng = np.random.default_rng(1)
        for what, mode, knobs in (("transpose", "T", {"explicit_transpose": 1}), ("colslab", "N", {"colslab": 2, "colslab_shift": 5})):
            nin, nout = (A0.nrows, A0.ncols) if mode == "T" else (A0.ncols, A0.nrows)
            x = rng.random(nin)
            for tracking in (0, 1, 2):
                A = dev(be, A0)
                h = kk.SPMVHandle("SPMV_DEFAULT")
                for k_, v_ in knobs.items(): h.set(k_, v_)
                h.set("values_tracking", tracking)
                xd, yd = be.from_numpy(x), be.from_numpy(np.zeros(nout))
                v = A0.values.copy()
                def run_and_check(tag):
                    kk.spmv(h, mode, 1.0, A, xd, 0.0, yd)
                    exp = oracle.spmv_sequential(mode, oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, v), 1.0, x, 0.0, np.zeros(nout))
                    np.testing.assert_allclose(be.to_numpy(yd), exp, rtol=1e-12, atol=1e-12, err_msg="%s tracking %d after %s" % (what, tracking, tag))
                run_and_check("the first call")
                assert h.query("transpose_cached" if mode == "T" else "colslab") == 1
                steps = (("one value", lambda: v.__setitem__(5000, -7.25)), ("every value", lambda: v.__imul__(3.0)),
                         ("a swap", lambda: v.__setitem__([0, len(v) - 1], v[[len(v) - 1, 0]])),
                         ("a tile negated", lambda: v.__setitem__(slice(4096, 8192), -v[4096:8192])),
                         ("a tile doubled", lambda: v.__setitem__(slice(8192, 12288), 2.0 * v[8192:12288])), ("nothing", lambda: None))
                for tag, change in steps:
                    change()
                    A.values[:] = be.from_numpy(v)
                    if tracking == 1 and tag != "nothing": h.values_changed()
                    run_and_check(tag)
                # a notification is harmless under the other policies, and a change of policy starts over
                h.values_changed(); run_and_check("a notification without a change")
                h.set("values_tracking", (tracking + 1) % 3)
                v[17] = 0.125; A.values[:] = be.from_numpy(v)
                if (tracking + 1) % 3 == 1: h.values_changed()
                run_and_check("a change of policy")
    finally:
        kk._capi.check(lib, lib.kkamd_set_default(b"explicit_transpose_min_knnz", 1000))


def check_entries_guard(be):
    """knob check_entries: a column array edited in place under a live handle is reported, an untouched one is not"""
    import pytest
    A0 = oracle.laplace3d("FE", 12, 11, 10)
    A = dev(be, A0)
    h = kk.SPMVHandle("SPMV_DEFAULT"); h.set("check_entries", 1)
    x, y = be.from_numpy(np.ones(A0.ncols)), be.from_numpy(np.zeros(A0.nrows))
    kk.spmv(h, "N", 1.0, A, x, 0.0, y); kk.spmv(h, "N", 1.0, A, x, 0.0, y)
    A.values[:] = be.from_numpy(A0.values * 2.0)                     # values may change
    kk.spmv(h, "N", 1.0, A, x, 0.0, y)
    e = be.to_numpy(A.graph.entries).copy(); e[5], e[6] = e[6], e[5]
    A.graph.entries[:] = be.from_numpy(e)                            # the structure may not
    with pytest.raises(kk.KkamdError) as ei:
        kk.spmv(h, "N", 1.0, A, x, 0.0, y)
    assert ei.value.status == kk._capi.ERR_STATE
    h2 = kk.SPMVHandle("SPMV_DEFAULT")                               # without the knob nothing is checked (and nothing is paid)
    kk.spmv(h2, "N", 1.0, A, x, 0.0, y)


def check_mv_transpose_cached(be, light=False):
    """Rank 2, modes T / H of an analysed handle run the mode-N dispatch on the cached transpose (no atomics): the four layout pairs,
    a value update between the calls, a lattice matrix (its transpose takes the plane-marching kernel), a rectangular one, 64-bit
    offsets; explicit_transpose 0 keeps the reference's atomic scatter."""
    lib = be.lib
    kk._capi.check(lib, lib.kkamd_set_default(b"explicit_transpose_min_knnz", 0))
    try:
        mats = ((oracle.random_crs(900, 700, 9, variance=3, seed=7, sorted_rows=True), 1.0), (oracle.laplace3d("FE", 34, 9, 8), 32.0))
        combos = list(zip((("C", "C"), ("F", "F"), ("C", "F"), ("F", "C")), (16, 5, 21, 32), (np.int32, np.int64, np.int32, np.int32)))
        if light:                                                  # the emulator: the unstructured matrix, two layout pairs (the GPU suite runs them all)
            mats, combos = mats[:1], combos[:2]
        for A0, maxv in mats:
            for (xo, yo), nvec, off in combos:
                h = check_spmv_mv(be, A0, nvec, "T", 1.5, 0.0, xo, yo, algo="SPMV_DEFAULT", max_val=maxv, nans=True, offset_dtype=off)
                assert h.query("transpose_cached") == 1
                check_spmv_mv(be, A0, nvec, "H", 1.0, -0.5, xo, yo, algo="SPMV_DEFAULT", max_val=maxv, offset_dtype=off)
        A0 = oracle.random_crs(900, 700, 9, variance=3, seed=7, sorted_rows=True)
        A = dev(be, A0)
        h = kk.SPMVHandle("SPMV_DEFAULT")
        rng = np.random.default_rng(4)
        X = rng.random((A0.nrows, 16)); v = A0.values.copy()
        for rep in range(3):
            Yd = _to_dev_2d(be, np.zeros((A0.ncols, 16)))
            kk.spmv(h, "T", 1.0, A, _to_dev_2d(be, X), 0.0, Yd)
            exp = oracle.spmv_mv_serial("T", oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, v), 1.0, X, 0.0, np.zeros((A0.ncols, 16)))
            np.testing.assert_allclose(_to_host_2d(be, Yd), exp, rtol=1e-12, atol=1e-12)
            v = rng.random(A0.nnz) - rep
            A.values[:] = be.from_numpy(v)
        h = check_spmv_mv(be, A0, 16, "T", 1.0, 0.5, "C", "C", algo="SPMV_DEFAULT", knobs={"explicit_transpose": 0})
        assert h.query("transpose_cached") == 0
    finally:
        kk._capi.check(lib, lib.kkamd_set_default(b"explicit_transpose_min_knnz", 1000))


def _to_dev_2d(be, M):
    """device 2-D array with the same logical layout (Fortran order kept through a transposed view)"""
    if be.name == "emu":
        return np.array(M, order="K", copy=True)
    import torch
    if M.flags.f_contiguous and not M.flags.c_contiguous:
        return torch.from_numpy(np.ascontiguousarray(M.T)).to("cuda").t()
    return torch.from_numpy(np.ascontiguousarray(M)).to("cuda")


def _to_host_2d(be, M):
    if be.name == "emu":
        return np.asarray(M)
    return M.detach().cpu().numpy()


def check_spgemm(be, A0, B0, offset_dtype=np.int32, reuse=True, value_dtype=np.float64, algo="SPGEMM_KK", options=None, expect_compressed=None):
    A, B = dev(be, A0, offset_dtype, value_dtype), dev(be, B0, offset_dtype, value_dtype)
    kh = kk.KokkosKernelsHandle(be)
    kh.create_spgemm_handle(algo)
    for k_, v_ in (options or {}).items():
        kh.get_spgemm_handle().set(k_, v_)
    Cm = kk.spgemm_symbolic(kh, A, False, B, False)
    Cgold = oracle.spgemm(A0, B0)
    rmC = be.to_numpy(Cm.graph.row_map).astype(np.int64)
    assert kh.get_spgemm_handle().get_c_nnz() == Cgold.nnz
    assert np.array_equal(rmC, Cgold.row_map), "symbolic row_map differs"
    if expect_compressed is not None:
        assert bool(kh.get_spgemm_handle().get(6)) == expect_compressed, "compression decision: %d (work %d of %d)" % (
            kh.get_spgemm_handle().get(6), kh.get_spgemm_handle().get(7), kh.get_spgemm_handle().get(1))
    kk.spgemm_numeric(kh, A, False, B, False, Cm)
    rm, ent, val = Cm.to_host()
    got = oracle.Crs(A0.nrows, B0.ncols, rm.astype(np.int64), ent, val.astype(np.float64))
    eps = 1e-7 if value_dtype == np.float64 else 3.7e-3
    if value_dtype != np.float64:
        Ag = oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, A0.values.astype(np.float32).astype(np.float64))
        Bg = oracle.Crs(B0.nrows, B0.ncols, B0.row_map, B0.entries, B0.values.astype(np.float32).astype(np.float64))
        Cgold = oracle.spgemm(Ag, Bg)
    ok, msg = oracle.is_same_matrix(got, Cgold, eps)
    assert ok, "spgemm: " + msg
    if reuse and A0.nnz and B0.nnz:
        # numeric again with new values on the same handle (Test_Sparse_spgemm.hpp:243-252)
        rng = np.random.default_rng(99)
        A2 = oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, 1 + 49 * rng.random(A0.nnz))
        Ad2 = kk.CrsMatrix(A0.nrows, A0.ncols, A.graph.row_map, A.graph.entries, be.from_numpy(A2.values.astype(value_dtype)), backend=be)
        kk.spgemm_numeric(kh, Ad2, False, B, False, Cm)
        rm, ent, val = Cm.to_host()
        got = oracle.Crs(A0.nrows, B0.ncols, rm.astype(np.int64), ent, val.astype(np.float64))
        if value_dtype != np.float64:
            A2 = oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, A2.values.astype(np.float32).astype(np.float64))
            Cg2 = oracle.spgemm(A2, Bg)
        else:
            Cg2 = oracle.spgemm(A2, B0)
        ok, msg = oracle.is_same_matrix(got, Cg2, eps)
        assert ok, "spgemm numeric reuse: " + msg
    kh.destroy_spgemm_handle()
    return got


def kept_structure_operands():
    """(A, B, Ad, Bd) of check_spgemm_kept_structure: hub lists of B over 400000 columns under short rows of A, and rows of C that are
    30 .. 100 % dense (kept bitmaps whose 64-word steps hold more than a wave's 1024 staging slots: halves, quarters)"""
    import fuzz_cases as fz
    rng = np.random.default_rng(5)
    n, k = 60, 400000
    B = fz.hubby(rng, n, k, 3000, 0, 3000)            # rows of B: 0 .. 6000 entries
    A = fz.hubby(rng, 10, n, 3, 2, 20)                # rows of A: 0 .. 6 entries, two of about 20
    kd = 8192
    lens = rng.integers(1500, 6000, size=30)
    rmd = np.zeros(31, dtype=np.int64); np.cumsum(lens, out=rmd[1:])
    Bd0 = oracle.Crs(30, kd, rmd, np.concatenate([np.sort(rng.choice(kd, size=l, replace=False)) for l in lens]).astype(np.int32), 1 + 49 * rng.random(rmd[-1]))
    rows_d = [np.sort(rng.choice(30, size=c, replace=False)) for c in (1, 2, 3, 6, 12, 30)]
    armd = np.zeros(len(rows_d) + 1, dtype=np.int64); np.cumsum([len(r) for r in rows_d], out=armd[1:])
    Ad0 = oracle.Crs(len(rows_d), 30, armd, np.concatenate(rows_d).astype(np.int32), 1 + 49 * rng.random(armd[-1]))
    return A, B, Ad0, Bd0


def check_spgemm_kept_structure(be):
    """The symbolic phase keeps, for the first numeric call, the bitmaps of its densest rows (>= k/32 entries) and the ENTRY LISTS of the
    other dense rows (round 4; lists above 6144 entries leave LDS in several rounds): structure identical to the oracle's, both sources
    used, numeric reuse keeps the entries, and with the lists switched off the same C comes out"""
    A, B, Ad0, Bd0 = kept_structure_operands()
    gold = oracle.spgemm(A, B)
    got_d = check_spgemm(be, Ad0, Bd0)
    assert np.diff(got_d.row_map).max() > 8000 and np.diff(got_d.row_map).min() >= 1500
    kh = kk.KokkosKernelsHandle(be); kh.create_spgemm_handle("SPGEMM_KK")
    Cd = kk.spgemm_symbolic(kh, dev(be, Ad0), False, dev(be, Bd0), False)
    kk.spgemm_numeric(kh, dev(be, Ad0), False, dev(be, Bd0), False, Cd)
    assert kh.get_spgemm_handle().get(12) >= 4, kh.get_spgemm_handle().get(12)          # written from kept bitmaps
    kh.destroy_spgemm_handle()
    for lists in (1, 0):
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_keep_lists", lists))
        try:
            kh = kk.KokkosKernelsHandle(be); kh.create_spgemm_handle("SPGEMM_KK")
            Ad, Bd = dev(be, A), dev(be, B)
            Cm = kk.spgemm_symbolic(kh, Ad, False, Bd, False)
            kk.spgemm_numeric(kh, Ad, False, Bd, False, Cm)
            sh = kh.get_spgemm_handle()
            assert sh.get(12) > 0 and (sh.get(14) > 0) == bool(lists), (sh.get(12), sh.get(14))
            rm, ent, val = Cm.to_host()
            ok, msg = oracle.is_same_matrix(oracle.Crs(A.nrows, B.ncols, rm.astype(np.int64), ent, val.astype(np.float64)), gold)
            assert ok, msg
            kk.spgemm_numeric(kh, Ad, False, Bd, False, Cm)            # reuse: entries kept
            assert sh.get(11) == 1
            rm2, ent2, val2 = Cm.to_host()
            assert np.array_equal(ent, ent2) and np.allclose(val, val2, rtol=1e-13)
            kh.destroy_spgemm_handle()
        finally:
            kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_keep_lists", 1))


def units_operands():
    """the three products of check_spgemm_units as [(A, B, name)], and the generator that drew them (the check goes on drawing from it):
    (a) hub lists next to short ones, k not a multiple of any window; (b) dense rows; (c) an A row of 700 lists (three chunks), B rows of
    0 .. 30 entries"""
    import fuzz_cases as fz
    rng = np.random.default_rng(61)
    n, k = 60, 100003
    B = fz.hubby(rng, n, k, 2500, 0, 2500)
    A = fz.hubby(rng, 10, n, 3, 2, 20)
    kd = 8192
    lens = rng.integers(1500, 6000, size=30)
    rmd = np.zeros(31, dtype=np.int64); np.cumsum(lens, out=rmd[1:])
    Bd = oracle.Crs(30, kd, rmd, np.concatenate([np.sort(rng.choice(kd, size=l, replace=False)) for l in lens]).astype(np.int32), 1 + 49 * rng.random(rmd[-1]))
    rows_d = [np.sort(rng.choice(30, size=c, replace=False)) for c in (1, 2, 3, 6, 12, 30)]
    armd = np.zeros(len(rows_d) + 1, dtype=np.int64); np.cumsum([len(r) for r in rows_d], out=armd[1:])
    Ad = oracle.Crs(len(rows_d), 30, armd, np.concatenate(rows_d).astype(np.int32), 1 + 49 * rng.random(armd[-1]))
    Bs = randomized(oracle.random_crs(900, 30000, 14, variance=14, seed=23, sorted_rows=True))
    cols = np.sort(rng.choice(900, size=700, replace=False)).astype(np.int32)
    As = oracle.Crs(3, 900, np.array([0, 700, 703, 1100]), np.concatenate([cols, [1, 5, 9], np.sort(rng.choice(900, size=397, replace=False))]).astype(np.int32), 1 + 49 * rng.random(1100))
    return [(A, B, "hubs"), (Ad, Bd, "dense"), (As, Bs, "many short lists")], rng


def check_spgemm_units(be, light=False):
    """Round 6: the symbolic phase counts its dense class by UNITS (row of C, window of 2^unit_bits columns; an index of B at window
    granularity cuts every list).  Windows of 64 .. 2^18 columns over products whose rows are sparse, dense, a single list, hundreds of
    lists (several chunks of 256), lists shorter than a quad, empty pieces in most windows; 32- and 64-bit offsets; with the bitmaps,
    the lists or both switched off; against the one-workgroup-per-row kernel (spgemm_sym_units 0).  Structure identical to the oracle's
    every time (check_spgemm), and the queries say the units were used."""
    setd = lambda key, v: kk._capi.check(be.lib, be.lib.kkamd_set_default(key, v))
    cases, rng = units_operands()
    (A, B, _), (Ad, Bd, _), _ = cases
    try:
        for bits in ((6, 12, 18) if light else (6, 9, 12, 15, 18)):
            setd(b"spgemm_unit_bits", bits)
            for A0, B0, name in cases:
                if bits == 6 and name == "hubs" : continue               # 1563 windows x 10 rows of one word each: slow under the emulator, nothing new
                for odt in (np.int32, np.int64):
                    got = check_spgemm(be, A0, B0, offset_dtype=odt, reuse=(bits == 12))
                kh = kk.KokkosKernelsHandle(be); kh.create_spgemm_handle("SPGEMM_KK")
                Am, Bm = dev(be, A0), dev(be, B0)
                Cm = kk.spgemm_symbolic(kh, Am, False, Bm, False)
                sh = kh.get_spgemm_handle()
                nwin = -(-B0.ncols // (1 << bits))
                assert sh.get(19) > 0 and sh.get(19) % nwin == 0, (name, bits, sh.get(19), nwin)          # class rows x windows
                assert sh.get(21) > 0 and sh.get(13) == sh.get(21), (name, bits, sh.get(21), sh.get(13))
                if name == "dense" and bits >= 9: assert sh.get(20) > 0, (bits, sh.get(20))               # units at least 1/32 dense keep bitmaps
                kk.spgemm_numeric(kh, Am, False, Bm, False, Cm)
                assert sh.get(12) > 0 and sh.get(13) == 0, (name, bits, sh.get(12), sh.get(13))
                kh.destroy_spgemm_handle()
        setd(b"spgemm_unit_bits", 10)
        for bm, ls in ((0, 1), (1, 0), (0, 0)):
            setd(b"spgemm_keep_bitmaps", bm); setd(b"spgemm_keep_lists", ls)
            for A0, B0, name in cases:
                check_spgemm(be, A0, B0, offset_dtype=np.int64, reuse=False)
        setd(b"spgemm_keep_bitmaps", 1); setd(b"spgemm_keep_lists", 1)
        setd(b"spgemm_sym_units", 0)                                      # the row-by-row kernel is still there (B with unsorted rows under several windows takes it)
        for A0, B0, name in cases:
            check_spgemm(be, A0, B0, reuse=False)
        setd(b"spgemm_sym_units", 1)
        # B with unsorted rows: one window -> units without an index; several windows -> row by row
        ent, val = B.entries.copy(), B.values.copy()
        for i in range(B.nrows):
            lo, hi = B.row_map[i], B.row_map[i + 1]
            q = rng.permutation(hi - lo)
            ent[lo:hi], val[lo:hi] = ent[lo:hi][q], val[lo:hi][q]
        Bu = oracle.Crs(B.nrows, B.ncols, B.row_map, ent, val)
        for bits in (18, 12):
            setd(b"spgemm_unit_bits", bits)
            check_spgemm(be, A, Bu, reuse=False)
        # a cap on the store (knob spgemm_store_cap_mb, for hosts that interleave their own allocations): room goes to the heaviest rows, the
        # others walk their products again in the numeric phase -- the same C; the queries report what the process-wide store holds and has held
        setd(b"spgemm_unit_bits", 12); setd(b"spgemm_store_cap_mb", 1)
        kk._capi.check(be.lib, be.lib.kkamd_release_scratch())
        kh = kk.KokkosKernelsHandle(be); kh.create_spgemm_handle("SPGEMM_KK")
        Am, Bm = dev(be, Ad), dev(be, Bd)
        Cm = kk.spgemm_symbolic(kh, Am, False, Bm, False)
        sh = kh.get_spgemm_handle()
        assert 0 < sh.get(22) <= 1 << 20 and sh.get(23) >= sh.get(22), (sh.get(22), sh.get(23))
        assert 0 < sh.get(21) < Ad.nrows, sh.get(21)                       # some rows complete, not all (the dense product wants 1.5 MB)
        kk.spgemm_numeric(kh, Am, False, Bm, False, Cm)
        rm_, ent_, val_ = Cm.to_host()
        ok, msg = oracle.is_same_matrix(oracle.Crs(Ad.nrows, Bd.ncols, rm_.astype(np.int64), ent_, val_.astype(np.float64)), oracle.spgemm(Ad, Bd))
        assert ok, msg
        kh.destroy_spgemm_handle()
    finally:
        setd(b"spgemm_store_cap_mb", 0)
        setd(b"spgemm_unit_bits", 18); setd(b"spgemm_keep_bitmaps", 1); setd(b"spgemm_keep_lists", 1); setd(b"spgemm_sym_units", 1)


def check_spgemm_pool_release(be):
    """The process-wide store of bitmaps / entry lists (GBs on large products) goes back to the device when the LAST SpGEMM handle is
    destroyed (round-4 review: a plain C caller kept it for ever); with "spgemm_pool_keep" 1 it outlives the handles and
    kkamd_release_scratch returns it.  Also: the store is sized by what the product can need, not by a flat share of the free memory."""
    import torch
    import fuzz_cases as fz
    rng = np.random.default_rng(5)
    n, k = 60, 400000
    B = fz.hubby(rng, n, k, 3000, 0, 3000)
    A = fz.hubby(rng, 10, n, 3, 2, 20)
    Ad, Bd = dev(be, A), dev(be, B)
    kk._capi.check(be.lib, be.lib.kkamd_release_scratch())
    torch.cuda.synchronize(); torch.cuda.empty_cache()

    def run(keep_a_second_handle=False):
        kh = kk.KokkosKernelsHandle(be); kh.create_spgemm_handle("SPGEMM_KK")
        other = None
        if keep_a_second_handle:
            other = kk.KokkosKernelsHandle(be); other.create_spgemm_handle("SPGEMM_KK")
        Cm = kk.spgemm_symbolic(kh, Ad, False, Bd, False)
        held = torch.cuda.mem_get_info()[0]                   # free memory while the handle holds its store
        kk.spgemm_numeric(kh, Ad, False, Bd, False, Cm)
        assert kh.get_spgemm_handle().get(12) + kh.get_spgemm_handle().get(14) > 0           # the store was used
        del Cm
        kh.destroy_spgemm_handle()
        return held, other

    kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_pool_keep", 2))       # always returned with the last handle
    try:
        free0 = torch.cuda.mem_get_info()[0]
        held, _ = run()
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        free1 = torch.cuda.mem_get_info()[0]
        assert free0 - held < (1 << 30), "store of %d MB for a product with 6e4 multiplications" % ((free0 - held) >> 20)    # (it was a tenth of the free HBM)
        assert free0 - free1 < (8 << 20), "the last handle is gone and %d MB are still held" % ((free0 - free1) >> 20)
        # a second live handle keeps the pool (the next product of the job will use it) until it is destroyed too
        _, other = run(keep_a_second_handle=True)
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        free2 = torch.cuda.mem_get_info()[0]
        other.destroy_spgemm_handle()
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        free3 = torch.cuda.mem_get_info()[0]
        assert free3 >= free2 and free0 - free3 < (8 << 20), (free0, free2, free3)
        # 1 = it outlives the handles until kkamd_release_scratch
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_pool_keep", 1))
        run()
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        free4 = torch.cuda.mem_get_info()[0]
        kk._capi.check(be.lib, be.lib.kkamd_release_scratch())
        torch.cuda.synchronize()
        free5 = torch.cuda.mem_get_info()[0]
        assert free5 >= free4 and free0 - free5 < (8 << 20), (free0, free4, free5)
        # 0 (default): whatever the process did before, after a release the next product's store is returned or kept -- and kkamd_release_scratch
        # always returns it
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_pool_keep", 0))
        run(); run()
        kk._capi.check(be.lib, be.lib.kkamd_release_scratch())
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        assert free0 - torch.cuda.mem_get_info()[0] < (8 << 20)
    finally:
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_pool_keep", 0))


def galerkin_operands(n):
    """27-point FE Laplacian n^3 (n even), P of a 2 x 2 x 2 aggregation (one entry per row), R = P^T and A P (by the oracle)"""
    A = oracle.laplace3d("FE", n, n, n)
    i = np.arange(n); c = n // 2
    ci = (i[:, None, None] // 2) * c * c + (i[None, :, None] // 2) * c + (i[None, None, :] // 2)
    nf = n ** 3
    P = oracle.Crs(nf, c ** 3, np.arange(nf + 1, dtype=np.int64), ci.reshape(-1).astype(np.int32), np.ones(nf))
    order = np.argsort(P.entries, kind="stable")                                       # R = P^T: coarse node -> its (up to) eight fine nodes
    rrm = np.zeros(c ** 3 + 1, dtype=np.int64); np.cumsum(np.bincount(P.entries, minlength=c ** 3), out=rrm[1:])
    R = oracle.Crs(c ** 3, nf, rrm, order.astype(np.int32), np.ones(nf))
    return A, P, R, oracle.spgemm(A, P)


def check_spgemm_galerkin(be):
    """The two products of a Galerkin coarse operator R A P (Test_Sparse_spgemm.hpp:491-504 lists rectangular shapes; the perf driver
    KokkosSparse_spgemm.cpp:372-423 takes any pair): A P -- 27 products and 1 .. 8 entries per row, a rectangular B with one entry per
    row -- and R (A P) -- up to 216 products and 27 entries per row: a product whose wave bin mixes the four-rows-per-wave kernels with the
    one-row kernels.  Structure bit-exact, values to 1e-7, numeric reuse, both offset widths."""
    A, P, R, AP = galerkin_operands(12)
    got = check_spgemm(be, A, P)
    assert got.nnz == AP.nnz
    C = check_spgemm(be, R, AP, offset_dtype=np.int64)
    assert 8 <= np.diff(C.row_map).min() and np.diff(C.row_map).max() == 27
    check_spgemm(be, R, AP, value_dtype=np.float32)


def block_kernel_operands():
    """(A, B) of check_spgemm_block_kernel"""
    rng = np.random.default_rng(23)
    n, k = 2600, 9000 + 37
    lens = rng.integers(0, 40, size=n); lens[:6] = (k, 3000, 2500, 0, 1, 700); lens[-1] = 1501
    rm = np.zeros(n + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
    ent = np.concatenate([np.sort(rng.choice(k, size=l, replace=False)) for l in lens]).astype(np.int32)
    B = oracle.Crs(n, k, rm, ent, 1 + 49 * rng.random(rm[-1]))
    rows = [np.arange(0, 2500),                          # 2500 lists, 100 % dense (contains row 0 of B)
            np.array([1, 2, 5, n - 1]),                  # four long lists: ~50 % dense
            np.arange(6, 700),                           # 694 short lists (more than the flat shapes take), ~2 entries per 256-column block ...
            np.array([3, 4]), np.array([n - 1]), np.array([], dtype=np.int64),
            np.sort(rng.choice(n, size=600, replace=False))]
    arm = np.zeros(len(rows) + 1, dtype=np.int64); np.cumsum([len(r) for r in rows], out=arm[1:])
    A = oracle.Crs(len(rows), n, arm, np.concatenate(rows).astype(np.int32), 1 + 49 * rng.random(arm[-1]))
    return A, B


def check_spgemm_block_kernel(be):
    """Column-block value kernel (round 5, `spgemm_block`): rows of C that are dense, or have more lists than the flat kernel's shapes
    hold, accumulate per (row, column block) in a direct-indexed LDS accumulator, with the pieces of every list taken from an index of
    B.  Cases: k not a multiple of the block width, blocks with no entry of a row, an A row of 2500 lists (three chunks of lists into
    one accumulator), a row that is 100 % dense, lists that end B's arrays (guarded 16-byte loads), empty B rows inside an A row,
    numeric reuse (the index of B is kept), 64-bit offsets and fp32.  Block widths 256 (many blocks), 4096 and the default."""
    A, B = block_kernel_operands()
    try:
        # items: groups of blocks with a position-indexed accumulator (cap: entries per group; 64 forces the dense blocks to stay column-indexed
        # items next to groups), or (items 0) one workgroup per (row, block)
        for w, odt, vdt, items, cap in ((256, np.int32, np.float64, 1, 6144), (256, np.int32, np.float64, 1, 64), (256, np.int64, np.float64, 1, 200),
                                        (4096, np.int64, np.float64, 1, 1000), (16384, np.int32, np.float32, 1, 6144), (256, np.int64, np.float32, 1, 100),
                                        (256, np.int32, np.float64, 0, 6144), (4096, np.int64, np.float32, 0, 6144)):
            kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_block_w", w))
            kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_items", items))
            kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_item_cap", cap))
            check_spgemm(be, A, B, offset_dtype=odt, value_dtype=vdt)
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_item_cap", 100))
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_items", 1))
        # the rows really went there (and stay away with the knob off: same C)
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_block_w", 1024))
        for on in (1, 0):
            kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_block", on))
            kh = kk.KokkosKernelsHandle(be); kh.create_spgemm_handle("SPGEMM_KK")
            Ad, Bd = dev(be, A), dev(be, B)
            Cm = kk.spgemm_symbolic(kh, Ad, False, Bd, False)
            kk.spgemm_numeric(kh, Ad, False, Bd, False, Cm)
            assert (kh.get_spgemm_handle().get(16) >= 3) == bool(on), kh.get_spgemm_handle().get(16)
            if on: assert kh.get_spgemm_handle().get(17) + kh.get_spgemm_handle().get(18) > 0, (kh.get_spgemm_handle().get(17), kh.get_spgemm_handle().get(18))
            rm_, ent_, val_ = Cm.to_host()
            ok, msg = oracle.is_same_matrix(oracle.Crs(A.nrows, B.ncols, rm_.astype(np.int64), ent_, val_.astype(np.float64)), oracle.spgemm(A, B))
            assert ok, msg
            if on:      # the (process-wide) knobs change under a live handle: numeric reuse rebuilds its indices and items for the new grid
                for w2, cap2 in ((256, 64), (4096, 6144)):
                    kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_block_w", w2))
                    kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_item_cap", cap2))
                    kk.spgemm_numeric(kh, Ad, False, Bd, False, Cm)
                    rm_, ent_, val_ = Cm.to_host()
                    ok, msg = oracle.is_same_matrix(oracle.Crs(A.nrows, B.ncols, rm_.astype(np.int64), ent_, val_.astype(np.float64)), oracle.spgemm(A, B))
                    assert ok, (w2, cap2, msg)
                kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_block_w", 1024))
                kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_item_cap", 100))
            kh.destroy_spgemm_handle()
    finally:
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_block", 1))
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_block_w", 16384))
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_items", 1))
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_item_cap", 6144))


def val_steps_operands():
    """A and [(last_len, B)] of check_spgemm_val_steps: the last row of B has last_len entries (nnz(B) is no multiple of 4)"""
    rng = np.random.default_rng(17)
    n, k = 400, 12000
    rows = [list(range(23)) + [n - 1],                    # 24 lists of ~6000 over 12000 columns: ~12 products per entry of C
            [0, 30, 31],                                  # one long list and two short ones
            list(range(20, 320)),                         # 300 lists: the 512-work-item shape
            [n - 1], [5], []]
    arm = np.zeros(len(rows) + 1, dtype=np.int64); np.cumsum([len(r) for r in rows], out=arm[1:])
    A = oracle.Crs(len(rows), n, arm, np.concatenate([np.array(r, dtype=np.int32) for r in rows]), 1 + 49 * rng.random(arm[-1]))

    def make_b(last_len):
        lens = np.concatenate([np.full(23, 6000), np.full(n - 24, 150), [last_len]])
        rm = np.zeros(n + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
        ent = np.concatenate([np.sort(rng.choice(k, size=l, replace=False)) for l in lens]).astype(np.int32)
        return oracle.Crs(n, k, rm, ent, 1 + 49 * rng.random(rm[-1]))
    return A, [(last_len, make_b(last_len)) for last_len in (6001, 6007, 6002)]


def check_spgemm_val_steps(be):
    """Flat value kernel (vector walk: units of eight entries of one list, 16-byte loads) on rows of C whose windows hold several steps of
    products (lists that overlap heavily), in the lightest shape (128 work-items), the 512-work-item shape (more than 256 lists) and next to
    rows whose windows end inside the first step.  The last row of B is one of the long lists and nnz(B) is not a multiple of 4: the 16-byte
    walks of the symbolic phase (unit kernel) and of the bitmap kernel take the array's last, partial quad from their tail registers.
    (The scalar walks with 1 .. 3 steps in flight, knob spgemm_val_steps, measured neutral in round 5, are gone in round 6.)"""
    A, Bs = val_steps_operands()
    for last_len, B in Bs:
        assert B.nnz % 4 == last_len % 4 != 0
        got = check_spgemm(be, A, B)
        assert np.diff(got.row_map)[0] > 5461
        for bits in (10, 12):                             # the unit kernel's windows cut the last list: its last piece ends the arrays
            kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_unit_bits", bits))
            try: check_spgemm(be, A, B, reuse=False)
            finally: kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_unit_bits", 18))
    check_spgemm(be, A, B, offset_dtype=np.int64, value_dtype=np.float32)


def sorted_emission_operands():
    """(A, B) of check_spgemm_sorted_emission"""
    rng = np.random.default_rng(23)
    nb, k = 3000, 50000
    lens = np.concatenate([np.full(1000, 3), np.full(2000, 20)])
    rm = np.zeros(nb + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
    ent = np.concatenate([np.sort(rng.choice(k, size=l, replace=False)) for l in lens]).astype(np.int32)
    B = oracle.Crs(nb, k, rm, ent, 1 + 49 * rng.random(rm[-1]))
    rows = []
    for i in range(40):
        rows.append(np.sort(rng.choice(np.arange(1000, 3000), size=int(rng.integers(20, 90)), replace=False)))    # 400 .. 1800 products
    rows.append(np.sort(rng.choice(1000, size=300, replace=False)))                                            # 300 lists of 3: two chunks
    rows.append(np.sort(rng.choice(np.arange(1000, 3000), size=102, replace=False)))                           # 2040 products: just inside
    rows.append(np.sort(rng.choice(np.arange(1000, 3000), size=104, replace=False)))                           # 2080: the bitmap kernel
    rows.append(np.sort(rng.choice(np.arange(1000, 3000), size=400, replace=False)))                           # 8000 products
    rows.append(np.array([5, 1500]))                                                                            # 23 products: wave kernel
    rows.append(np.array([], dtype=np.int64))
    rows.append(np.concatenate([np.full(1, 1200), np.sort(rng.choice(np.arange(1000, 3000), size=30, replace=False))]))   # (unsorted A row, maybe a duplicate column)
    arm = np.zeros(len(rows) + 1, dtype=np.int64); np.cumsum([len(r) for r in rows], out=arm[1:])
    A = oracle.Crs(len(rows), nb, arm, np.concatenate(rows).astype(np.int32), 1 + 49 * rng.random(arm[-1]))
    return A, B


def check_spgemm_sorted_emission(be):
    """Rows of C with more than 256 entries out of at most 2048 products: entries(C) sorted in LDS (`spgemm_emit_sort`, default) instead
    of walking the products through a 2^20-column bitmap.  A rows of more than 256 entries (two chunks of lists), duplicates among
    the products, rows above the product limit next to them (bitmap kernel), short rows (wave kernel); same C with the knob off."""
    A, B = sorted_emission_operands()
    gold = oracle.spgemm(A, B)
    sizes = np.diff(gold.row_map)
    assert (sizes[:42] > 256).all()
    for on in (1, 0):
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_emit_sort", on))
        try:
            for odt in (np.int32, np.int64):
                kh = kk.KokkosKernelsHandle(be); kh.create_spgemm_handle("SPGEMM_KK")
                Ad, Bd = dev(be, A, offset_dtype=odt), dev(be, B, offset_dtype=odt)
                Cm = kk.spgemm_symbolic(kh, Ad, False, Bd, False)
                kk.spgemm_numeric(kh, Ad, False, Bd, False, Cm)
                sh = kh.get_spgemm_handle()
                assert (sh.get(15) >= 42) == bool(on), sh.get(15)
                rm_, ent_, val_ = Cm.to_host()
                ok, msg = oracle.is_same_matrix(oracle.Crs(A.nrows, B.ncols, rm_.astype(np.int64), ent_, val_.astype(np.float64)), gold)
                assert ok, msg
                kk.spgemm_numeric(kh, Ad, False, Bd, False, Cm)            # reuse: entries kept
                assert sh.get(11) == 1
                rm2, ent2, val2 = Cm.to_host()
                assert np.array_equal(ent_, ent2) and np.allclose(val_, val2, rtol=1e-13)
                kh.destroy_spgemm_handle()
        finally:
            kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_emit_sort", 1))


def quad_rows_cases():
    """[(A, B)] of check_spgemm_quad_rows; the first is the 7-point stencil squared"""
    rng = np.random.default_rng(29)
    cases = []
    A7 = randomized(oracle.laplace3d("FD", 9, 7, 5)); cases.append((A7, A7))                      # 315 rows, 49 products at most
    A9 = randomized(oracle.laplace2d("FE", 13, 11)); cases.append((A9, A9))                       # 143 rows, 81 products: above the limit, wave path
    # restriction-like P (1 .. 3 entries per row) and A P: 7 .. 81 products per row, 3 .. 40 entries
    A27 = randomized(oracle.laplace3d("FE", 9, 7, 5))
    lens = rng.integers(1, 4, size=A27.ncols)
    rm = np.zeros(A27.ncols + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
    P = oracle.Crs(A27.ncols, 60, rm, np.concatenate([np.sort(rng.choice(60, size=l, replace=False)) for l in lens]).astype(np.int32), 1 + 49 * rng.random(rm[-1]))
    cases.append((A27, P))
    # mixed: every fifth row of A is long (200 entries on 1-entry rows of B: 200 products, two chunks of 16 do not apply -- wave path), the others tiny;
    # and a row of 40 entries on 1-entry rows (40 products, three chunks of a group)
    nb = 500
    B1 = oracle.Crs(nb, 4000, np.arange(nb + 1, dtype=np.int64), rng.integers(0, 4000, size=nb).astype(np.int32), 1 + 49 * rng.random(nb))
    rows = []
    for i in range(41):
        if i % 5 == 4: rows.append(np.sort(rng.choice(nb, size=200, replace=False)))
        elif i == 7: rows.append(np.sort(rng.choice(nb, size=40, replace=False)))
        elif i == 11: rows.append(np.array([], dtype=np.int64))
        else: rows.append(np.sort(rng.choice(nb, size=int(rng.integers(1, 17)), replace=False)))
    arm = np.zeros(len(rows) + 1, dtype=np.int64); np.cumsum([len(r) for r in rows], out=arm[1:])
    Am = oracle.Crs(len(rows), nb, arm, np.concatenate(rows).astype(np.int32), 1 + 49 * rng.random(arm[-1]))
    cases.append((Am, B1))
    return cases


def check_spgemm_quad_rows(be):
    """Wave-per-row kernels with four rows of the list per wave (`spgemm_quad_rows`): stencil products whose rows all have a few
    dozen products (16 lanes per row), lists whose length is no multiple of four, waves that mix small and larger rows (they fall back to
    one row after the other), A rows of more than 16 entries on 1-entry rows of B (two chunks per group), empty rows; same C with the knob off."""
    cases = quad_rows_cases()
    A7 = cases[0][0]
    try:
        for on in (2, 1, 0):         # 2: always (waves with a larger row fall back), 1: only when every row of the product is small (default), 0: never
            kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_quad_rows", on))
            for A, B in cases:
                check_spgemm(be, A, B)
            check_spgemm(be, A7, A7, offset_dtype=np.int64, value_dtype=np.float32)
    finally:
        kk._capi.check(be.lib, be.lib.kkamd_set_default(b"spgemm_quad_rows", 1))


def all_bins_operands():
    """(A, B) of test_spgemm_all_bins: rows landing in every launch shape of both phases: flops 0 / <=1365 / <=2048 / <=16384 / dense,
    and nnz(C row) <=256 / <=2048 / <=5461 / dense; row 6 is the union of three hub rows (dense path with overlapping columns)"""
    B0 = hub_matrix(64, 30000, 40, {0: 9000, 1: 3000, 2: 600, 3: 120, 5: 20000}, seed=1)
    rng = np.random.default_rng(2)
    cols_for = {0: [0], 1: [1], 2: [2], 3: [3, 7], 4: [], 5: [5], 6: [0, 1, 5], 7: list(range(6, 36))}
    rm = [0]; ent = []
    for i in range(8):
        ent += cols_for[i]; rm.append(len(ent))
    A0 = oracle.Crs(8, 64, np.array(rm), np.array(ent, dtype=np.int32), 1 + 49 * rng.random(len(ent)))
    return A0, B0


def dense_row_windows_operands():
    """(A0, B0, A1, B1, A2, B2, rng) of test_spgemm_dense_row_windows: hub rows of B under short rows of A; an A row of 650 entries (longer than
    the LDS cursor cache of 512); an A row of 2500 entries (above the row-flops pass's workgroup-per-row threshold) next to short ones"""
    B0 = hub_matrix(48, 26000, 25, {0: 9000, 1: 7000, 2: 12000, 3: 300}, seed=11)
    rm = [0, 3, 4, 8, 8, 11]
    ent = np.array([0, 1, 2,   2,   0, 3, 5, 9,   1, 2, 30], dtype=np.int32)
    rng = np.random.default_rng(3)
    A0 = oracle.Crs(5, 48, np.array(rm), ent, 1 + 49 * rng.random(len(ent)))
    B1 = randomized(oracle.random_crs(700, 20000, 12, variance=6, seed=21, sorted_rows=True))
    cols = np.sort(rng.choice(700, size=650, replace=False)).astype(np.int32)
    A1 = oracle.Crs(2, 700, np.array([0, 650, 653]), np.concatenate([cols, [1, 5, 9]]).astype(np.int32), 1 + 49 * rng.random(653))
    B2 = randomized(oracle.random_crs(3000, 5000, 3, variance=2, seed=22, sorted_rows=True))
    cols2 = np.sort(rng.choice(3000, size=2500, replace=False)).astype(np.int32)
    A2 = oracle.Crs(3, 3000, np.array([0, 2, 2502, 2505]), np.concatenate([[4, 7], cols2, [1, 5, 9]]).astype(np.int32), 1 + 49 * rng.random(2505))
    return A0, B0, A1, B1, A2, B2, rng


def randomized(A0, seed=5):
    """values re-drawn in [1,50) as the reference's SpGEMM tests do (Test_Sparse_spgemm.hpp:62-72)"""
    rng = np.random.default_rng(seed)
    return oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, 1 + 49 * rng.random(A0.nnz))


def hub_matrix(n, ncols, base_nnz, hubs, seed=0):
    """sorted random matrix with a few very long rows: rows i in `hubs` get hubs[i] entries"""
    rng = np.random.default_rng(seed)
    lens = np.full(n, base_nnz)
    for i, l in hubs.items():
        lens[i] = l
    rm = np.zeros(n + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
    ent = np.empty(rm[-1], dtype=np.int32)
    for i in range(n):
        ent[rm[i]:rm[i + 1]] = np.sort(rng.choice(ncols, size=lens[i], replace=False))
    return oracle.Crs(n, ncols, rm, ent, 1 + 49 * rng.random(rm[-1]))


# ------------------------------------------------------------------------------------------- SpGEMM: values, exactly
# check_spgemm compares values with the reference's relative comparator (1e-7 / 3.7e-3 on non-negative inputs).  The checks below
# compare them with a plain numpy reference of their own (spgemm_by_products, long-double sums), bit for bit where the inputs make
# every partial sum exactly representable (check_spgemm_exact) and within the textbook bound where they do not (mode "bound"), and
# read the library's "verbose" lines to prove which value kernel every case reached.
U_ROUND = {np.dtype(np.float64): 2.0 ** -53, np.dtype(np.float32): 2.0 ** -24}
P_BITS = {np.dtype(np.float64): 53, np.dtype(np.float32): 24}
# the numeric phase's bins (first "verbose" line) and its value kernels (second line), in the order the library prints them
BIN_COUNTS = ("wave hash", "block hash small", "block hash large", "dense rows", "column blocks", "LDS value windows", "LDS hub windows", "HBM accumulator")
VALUE_KERNELS = ("quad", "wave", "block_small", "block_large", "items_rank", "items_direct", "blocks_wg", "win128", "win256", "win512", "win1024",
                 "hub", "hub_multi", "hbm")
KNOB_DEFAULTS = {"spgemm_block_w": 16384, "spgemm_items": 1, "spgemm_item_cap": 6144, "spgemm_quad_rows": 1, "spgemm_force_unsorted": 0,
                 "spgemm_val_cap": 2048, "spgemm_unit_bits": 18, "spgemm_win_bits": 1 << 20, "spgemm_emit_sort": 1, "spgemm_block": 1}
# switches whose other setting selected code the library never ran by default: they went, with that code
REMOVED_SPGEMM_KNOBS = ("spgemm_val_kernel", "spgemm_val_shape", "spgemm_val_hub_flat", "spgemm_val_mid", "spgemm_hub_chunked", "spgemm_val_la",
                        "spgemm_val_la2", "spgemm_hub_split", "spgemm_nt", "spgemm_sort_rows", "spgemm_list_staged", "spgemm_emit_staged",
                        "spgemm_sym_large", "spgemm_col_quads")


def check_spgemm_knob_keys(be):
    """kkamd_set_default: every removed SpGEMM switch is an unknown key now (KKAMD_ERR_INVALID_ARG, at either setting), and every knob
    the exact-value cases set is still accepted"""
    for key in REMOVED_SPGEMM_KNOBS:
        for value in (0, 1, 2):
            status = be.lib.kkamd_set_default(key.encode(), value)
            assert status == kk._capi.ERR_INVALID_ARG, (key, value, status)
            assert "unknown key" in be.lib.kkamd_last_error().decode(errors="replace"), key
    for key, value in KNOB_DEFAULTS.items():
        kk._capi.check(be.lib, be.lib.kkamd_set_default(key.encode(), value))


class ProductsOf:
    """the expanded products of A * B, stable-sorted by (row, column): which entry of A and of B makes each product, where every entry of C
    begins, and the structure of C (row_map int64, entries int32, n = products per entry)"""

    def __init__(self, A0, B0):
        assert A0.ncols == B0.nrows
        lenB = np.diff(B0.row_map)
        cnt = lenB[A0.entries] if A0.nnz else np.zeros(0, dtype=np.int64)           # products of every entry of A
        total = int(cnt.sum())
        self.a_idx = np.repeat(np.arange(A0.nnz, dtype=np.int64), cnt)
        begin = np.cumsum(cnt) - cnt
        self.b_idx = np.repeat(B0.row_map[:-1][A0.entries] - begin, cnt) + np.arange(total, dtype=np.int64) if total else np.zeros(0, dtype=np.int64)
        row_of_a = np.repeat(np.arange(A0.nrows, dtype=np.int64), np.diff(A0.row_map))
        rows = row_of_a[self.a_idx]
        key = rows * np.int64(max(B0.ncols, 1)) + B0.entries[self.b_idx]
        order = np.argsort(key, kind="stable")
        self.a_idx, self.b_idx, key = self.a_idx[order], self.b_idx[order], key[order]
        self.first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if total else np.zeros(0, dtype=np.int64)
        self.n = np.diff(np.concatenate([self.first, [total]])).astype(np.int64)
        self.entries = (key[self.first] % max(B0.ncols, 1)).astype(np.int32)
        self.row_map = np.zeros(A0.nrows + 1, dtype=np.int64)
        np.cumsum(np.bincount(key[self.first] // max(B0.ncols, 1), minlength=A0.nrows), out=self.row_map[1:])
        self.n_max = int(self.n.max()) if total else 0

    def reduce(self, valA, valB):
        """per entry of C: (sum of its products, S = sum of their magnitudes), accumulated in np.longdouble in the sorted order"""
        assert np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant, "np.longdouble is no wider than float64 here"
        if not self.first.size:
            return np.zeros(0, dtype=np.longdouble), np.zeros(0, dtype=np.longdouble)
        with np.errstate(invalid="ignore", over="ignore"):
            prod = valA.astype(np.longdouble)[self.a_idx] * valB.astype(np.longdouble)[self.b_idx]
            return np.add.reduceat(prod, self.first), np.add.reduceat(np.abs(prod), self.first)


def spgemm_by_products(A0, B0):
    """C = A * B by its definition, independent of the oracle: every product (row, column, a * b) expanded, stable-sorted by (row, column) and
    reduced per entry in np.longdouble.  Rows of A and B need not be sorted and may hold a column several times (every pair of duplicates
    contributes its own product).  Returns (row_map, entries, sums, n, S): C's structure as the library writes it (rows column-sorted, every
    structural entry kept, a sum that cancels included) and per entry the sum, the number of products and S = sum |a * b|."""
    P = ProductsOf(A0, B0)
    sums, S = P.reduce(np.asarray(A0.values, dtype=np.float64), np.asarray(B0.values, dtype=np.float64))
    return P.row_map, P.entries, sums, P.n, S


def value_bits(n_max, value_dtype):
    """b: with values that are integers below 2^b times a fixed power of two, a product has at most 2b bits and a sum of at most n_max
    products 2b + ceil(log2 n_max): while that is at most P - 1 every partial sum, in any order, fused or not, is exactly representable"""
    return min(20, (P_BITS[np.dtype(value_dtype)] - 1 - int(math.ceil(math.log2(max(n_max, 1))))) // 2)


def exact_values(rng, size, b):
    """signed integers of at most b bits (never zero) times 2^-4"""
    mag = rng.integers(1, 1 << b, size=size).astype(np.float64)
    return np.where(rng.random(size) < 0.5, -mag, mag) * 2.0 ** -4


def _with_values(A0, values):
    return oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, values)


CANCEL_KEEP = 4          # cancelling mode: columns c with c % CANCEL_KEEP == 1 keep re-drawn values, the others cancel


def cancelling_pair(A0, B0):
    """the structures A' = [A A] (every row's entries, then the same entries n columns further) and B' = B stacked on a copy of B"""
    lenA = np.diff(A0.row_map)
    pos = np.arange(A0.nnz, dtype=np.int64)
    row = np.repeat(np.arange(A0.nrows, dtype=np.int64), lenA)
    within = pos - A0.row_map[:-1][row]
    dst1 = 2 * A0.row_map[:-1][row] + within
    dst2 = dst1 + lenA[row]
    ent = np.empty(2 * A0.nnz, dtype=np.int32)
    ent[dst1] = A0.entries; ent[dst2] = A0.entries + A0.ncols
    A2 = oracle.Crs(A0.nrows, 2 * A0.ncols, 2 * A0.row_map, ent, np.zeros(2 * A0.nnz))
    rmB = np.concatenate([B0.row_map, B0.row_map[1:] + B0.row_map[-1]])
    B2 = oracle.Crs(2 * B0.nrows, B0.ncols, rmB, np.concatenate([B0.entries, B0.entries]), np.zeros(2 * B0.nnz))
    return A2, B2, dst1, dst2


SPECIALS = (0.0, np.inf, -np.inf, np.nan)


def special_positions(rng, A0, extra):
    """positions of the array that get a special value: its first and last entry, the first and the last entry of a row in the middle and of
    the longest row, and `extra` random ones"""
    if A0.nnz == 0:
        return np.zeros(0, dtype=np.int64)
    lens = np.diff(A0.row_map)
    rows = np.flatnonzero(lens)
    mid, longest = rows[len(rows) // 2], int(np.argmax(lens))
    pos = [0, A0.nnz - 1, A0.row_map[mid], A0.row_map[mid + 1] - 1, A0.row_map[longest], A0.row_map[longest + 1] - 1]
    pos += list(rng.integers(0, A0.nnz, size=extra))
    return np.array(pos, dtype=np.int64)


def parse_numeric_verbose(out):
    """({bin: rows}, {value kernel: rows}) of the last numeric call's two "verbose" lines in `out`"""
    bins = re.findall(r"kkamd spgemm numeric \((\w+)\): rows per kernel -- (.*)", out)
    kern = re.findall(r"kkamd spgemm numeric \((\w+)\): rows per value kernel -- (.*)", out)
    assert bins and kern, "no verbose lines of the numeric phase in: %r" % out[-400:]
    nums = [int(v) for v in re.findall(r"\d+", bins[-1][1])]
    assert len(nums) == len(BIN_COUNTS), bins[-1]
    kd = {k_: int(v_) for k_, v_ in re.findall(r"(\w+)=(\d+)", kern[-1][1])}
    assert set(kd) == set(VALUE_KERNELS) | {"blocks"}, kern[-1]
    kd["dense_alg"] = int(kern[-1][0] == "SPGEMM_KK_DENSE")
    return dict(zip(BIN_COUNTS, nums)), kd


class Coverage:
    """which bins and value kernels a set of cases has reached, and (mode "bound") the largest error / bound seen next to each kernel"""

    def __init__(self):
        self.bins = {k_: 0 for k_ in BIN_COUNTS}
        self.kernels = {k_: 0 for k_ in VALUE_KERNELS + ("dense_alg", "emit_sorted")}
        self.ratio = {k_: 0.0 for k_ in VALUE_KERNELS + ("dense_alg",)}

    def add(self, bins, kernels, ratio=None):
        for k_, v_ in bins.items(): self.bins[k_] += v_
        for k_, v_ in kernels.items():
            self.kernels[k_] += v_
            if v_ and ratio is not None and k_ in self.ratio: self.ratio[k_] = max(self.ratio[k_], ratio)

    def assert_complete(self, what):
        missing = [k_ for k_, v_ in self.bins.items() if not v_] + [k_ for k_, v_ in self.kernels.items() if not v_]
        assert not missing, "%s: no case reached %s (bins %r, kernels %r)" % (what, missing, self.bins, self.kernels)


def check_spgemm_exact(be, A0, B0, mode="signed", offset_dtype=np.int32, value_dtype=np.float64, algo="SPGEMM_KK", knobs=None, capfd=None,
                       expect=(), coverage=None, seed=0, name=""):
    """C = A * B on the STRUCTURE of A0 and B0 with values drawn here, against spgemm_by_products.  Structure bit for bit; values by mode:
      signed      signed integers of b bits times 2^-4, b from the case (value_bits): every order of summation gives the same bits: `==`
      cancelling  A' = [A A], B' = B over a copy of B whose values are the negated ones in three columns out of four: those entries of C are
                  sums of at least two products that are exactly zero -- they must be present and hold 0; at least a tenth of nnz(C) are
                  such; everything else `==`
      special     +Inf, -Inf, NaN and stored 0.0 written into A and B (first / last entry of the arrays and of rows among them): NaN where the
                  reference has NaN, the same infinity where it has one, `==` elsewhere; then numeric reuse on the same handle with finite
                  values must be `==` again (nothing non-finite may survive in a table, an accumulator or a store)
      bound       signed real values, uniform in (-50, 50) and rounded to the value type: |C - reference| <= gamma_(n+1) S per entry, gamma_m =
                  m u / (1 - m u), u the unit roundoff of the value type, n and S the entry's number of products and sum of |a * b| -- the bound
                  of any order of summation of n rounded products (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1), plus
                  the reference's own error (the same expression with the long double's unit roundoff)
    knobs: process-wide defaults set for the case and restored.  capfd: the library's verbose lines are read, the rows per bin and value kernel
    are added to `coverage`, and every kernel named in `expect` must have taken rows.  Returns the largest error / bound (mode "bound") or 0."""
    vdt = np.dtype(value_dtype)
    rng = np.random.default_rng([seed, 17])
    if mode == "cancelling":
        A0, B0, dst1, dst2 = cancelling_pair(A0, B0)
    P = ProductsOf(A0, B0)
    b = value_bits(P.n_max, vdt)
    assert b >= (13 if vdt == np.float64 else 3), "%s: %d products meet in one entry: %d-bit values cannot tell a rounding apart" % (name, P.n_max, b)

    def draw():
        if mode == "bound":
            return (rng.uniform(-50, 50, A0.nnz).astype(vdt).astype(np.float64), rng.uniform(-50, 50, B0.nnz).astype(vdt).astype(np.float64))
        va, vb = exact_values(rng, A0.nnz, b), exact_values(rng, B0.nnz, b)
        if mode == "cancelling":
            half = B0.nnz // 2
            va[dst2] = va[dst1]
            cancels = B0.entries[:half] % CANCEL_KEEP != 1
            vb[half:][cancels] = -vb[:half][cancels]
        return va, vb
    va, vb = draw()
    if mode == "special":
        for v, M in ((va, A0), (vb, B0)):
            pos = special_positions(rng, M, extra=min(48, 2 + M.nnz // 64))
            v[pos] = np.array(SPECIALS)[np.arange(len(pos)) % 4]
    assert np.array_equal(va.astype(vdt).astype(np.float64), va, equal_nan=True) and np.array_equal(vb.astype(vdt).astype(np.float64), vb, equal_nan=True)
    if knobs:
        for k_, v_ in knobs.items(): kk._capi.check(be.lib, be.lib.kkamd_set_default(k_.encode(), v_))
    try:
        A, B = dev(be, _with_values(A0, va), offset_dtype, vdt), dev(be, _with_values(B0, vb), offset_dtype, vdt)
        kh = kk.KokkosKernelsHandle(be)
        kh.create_spgemm_handle(algo)
        sh = kh.get_spgemm_handle()
        Cm = kk.spgemm_symbolic(kh, A, False, B, False)
        assert np.array_equal(be.to_numpy(Cm.graph.row_map).astype(np.int64), P.row_map), name + ": symbolic row_map differs from the products'"
        if capfd is not None:
            capfd.readouterr(); sh.set("verbose", 1)
        kk.spgemm_numeric(kh, A, False, B, False, Cm)
        if capfd is not None:
            sh.set("verbose", 0)
            bins, kernels = parse_numeric_verbose(capfd.readouterr().out)
            assert kernels["dense_alg"] == int(sh.get(8) == 1)
            kernels["emit_sorted"] = sh.get(15)                          # rows whose entries(C) were sorted in LDS (a structure kernel; the handle counts it)
            blocks = kernels.pop("blocks")                                # the handle's own queries say the same
            assert blocks == (sh.get(16) if bins["dense rows"] else 0) == bins["column blocks"], (kernels, sh.get(16))
            if blocks and not kernels["blocks_wg"]: assert (kernels["items_rank"], kernels["items_direct"]) == (sh.get(17), sh.get(18)), (kernels, sh.get(17), sh.get(18))
            for k_ in expect:                                             # a dict: exactly that many rows
                assert kernels[k_] == expect[k_] if isinstance(expect, dict) else kernels[k_] > 0, "%s: rows of the value kernel %r: %r" % (name, k_, kernels)
        ratio = _compare_exact(P, va, vb, Cm, mode, vdt, name)
        if mode == "special":                                       # numeric reuse: finite values into the same arrays of A and B's graph, same handle, same C
            va2, vb2 = exact_values(rng, A0.nnz, b), exact_values(rng, B0.nnz, b)
            A2 = kk.CrsMatrix(A0.nrows, A0.ncols, A.graph.row_map, A.graph.entries, be.from_numpy(va2.astype(vdt)), backend=be)
            B2 = kk.CrsMatrix(B0.nrows, B0.ncols, B.graph.row_map, B.graph.entries, be.from_numpy(vb2.astype(vdt)), backend=be)
            kk.spgemm_numeric(kh, A2, False, B2, False, Cm)
            _compare_exact(P, va2, vb2, Cm, "signed", vdt, name + " (numeric reuse after the special values)")
        kh.destroy_spgemm_handle()
    finally:
        if knobs:
            for k_ in knobs: kk._capi.check(be.lib, be.lib.kkamd_set_default(k_.encode(), KNOB_DEFAULTS[k_]))
    if capfd is not None and coverage is not None:
        coverage.add(bins, kernels, ratio if mode == "bound" else None)
    return ratio


def _compare_exact(P, va, vb, Cm, mode, vdt, name):
    rm, ent, val = Cm.to_host()
    nnz = int(P.row_map[-1])
    assert np.array_equal(rm.astype(np.int64), P.row_map), name + ": row_map differs"
    assert np.array_equal(ent[:nnz], P.entries), name + ": entries differ"
    got = val[:nnz].astype(np.float64)
    sums, S = P.reduce(va, vb)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = sums.astype(np.float64)

    def first_bad(bad):
        i = int(np.flatnonzero(bad)[0]); r = int(np.searchsorted(P.row_map, i, side="right") - 1)
        return "%d entries, first at row %d column %d (%d products): %r, reference %r" % (int(bad.sum()), r, int(P.entries[i]), int(P.n[i]), got[i], ref[i])
    if mode == "bound":
        u = U_ROUND[vdt]; ul = float(np.finfo(np.longdouble).eps) / 2
        m = (P.n + 1).astype(np.longdouble)
        bound = (m * u / (1 - m * u) + m * ul / (1 - m * ul)) * S
        err = np.abs(got.astype(np.longdouble) - sums)
        bad = ~(err <= bound)
        assert not bad.any(), name + ": outside the bound gamma_(n+1) S: " + first_bad(bad)
        return float((err / bound).max()) if nnz else 0.0
    assert (ref == sums).all() or mode == "special", name + ": the reference's sums are not representable in float64 (the case's b is wrong)"
    if mode == "special":
        nan = np.isnan(ref)
        assert nan.any() and np.isinf(ref).any() and (np.isfinite(ref).sum() >= nnz // 8), name + ": the special values reach %d NaN, %d Inf of %d entries" % (int(nan.sum()), int(np.isinf(ref).sum()), nnz)
        bad = np.isnan(got) != nan
        assert not bad.any(), name + ": NaN positions differ: " + first_bad(bad)
        fin = np.isfinite(ref)
        assert ((ref == sums) | ~fin).all(), name + ": a finite reference sum is not representable in float64"
        bad = ~nan & (got != ref)
        assert not bad.any(), name + ": values differ (Inf or finite entries): " + first_bad(bad)
        return 0.0
    bad = got != ref
    assert not bad.any(), name + ": values differ: " + first_bad(bad)
    if mode == "cancelling":
        zero = P.entries % CANCEL_KEEP != 1
        assert (P.n[zero] >= 2).all() and (ref[zero] == 0).all() and zero.sum() * 10 >= nnz > 0, name + ": %d cancelling entries of %d" % (int(zero.sum()), nnz)
        assert (got[zero] == 0).all()
    return 0.0


def limit_operands(seed=41):
    """(A, B): rows exactly at the limits the numeric dispatcher uses.  B has a million columns (no row of C is dense enough for the column-block
    class): rows 0 .. 999 of exactly 8 entries, rows 1000 .. 2999 of exactly 1 entry in columns of their own, the others 1 .. 3 entries.
    Rows of A: 256 / 257 one-entry lists (256 / 257 entries of C: wave table / dense bin); 32 / 33 one-entry lists (four rows per wave / one);
    8 eight-entry lists (64 products) and one more one-entry list (65); 128 / 129 eight-entry lists (value windows of 128 / 256 work-items); 256 eight-entry lists (2048 products) and one more (2049); 512 / 513,
    1024 / 1025 and 4096 / 4097 entries (value windows of 512 and of 1024 work-items, hub kernel in one pass and in two), 9000 (three passes),
    3 entries and none."""
    rng = np.random.default_rng(seed)
    nB, k = 14000, 1000003
    lens = rng.integers(1, 4, size=nB); lens[:1000] = 8; lens[1000:3000] = 1
    rm = np.zeros(nB + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
    ent = np.concatenate([np.sort(rng.choice(k, size=l, replace=False)) for l in lens]).astype(np.int32)
    ent[rm[1000]:rm[3000]] = rng.choice(k, size=2000, replace=False)
    B = oracle.Crs(nB, k, rm, ent, np.ones(rm[-1]))
    ones, eights, rest = np.arange(1000, 3000), np.arange(0, 1000), np.arange(3000, nB)
    pick = lambda pool, c: np.sort(rng.choice(pool, size=c, replace=False))
    rows = [pick(eights, 128), pick(eights, 129), pick(ones, 256), pick(ones, 257), pick(ones, 32), pick(ones, 33), pick(eights, 8), np.concatenate([pick(eights, 8), pick(ones, 1)]),
            pick(eights, 256), np.concatenate([pick(eights, 256), pick(ones, 1)]), pick(rest, 512), pick(rest, 513), pick(rest, 1024), pick(rest, 1025),
            pick(rest, 4096), pick(rest, 4097), pick(rest, 9000), pick(rest, 3), np.array([], dtype=np.int64)]
    arm = np.zeros(len(rows) + 1, dtype=np.int64); np.cumsum([len(r) for r in rows], out=arm[1:])
    A = oracle.Crs(len(rows), nB, arm, np.concatenate(rows).astype(np.int32), np.ones(arm[-1]))
    return A, B


def unsorted_rows(B0, seed=3):
    """B0 with the entries of every row in a random order"""
    rng = np.random.default_rng(seed)
    ent = B0.entries.copy()
    for i in range(B0.nrows):
        lo, hi = B0.row_map[i], B0.row_map[i + 1]
        ent[lo:hi] = ent[lo:hi][rng.permutation(hi - lo)]
    return oracle.Crs(B0.nrows, B0.ncols, B0.row_map, ent, B0.values)


def exact_cases(light=False):
    """[(name, A, B, algo, knobs, value kernels the case must reach, or {kernel: rows})]: the structures of the SpGEMM checks of this file, with the knob settings
    those checks use, and rows at the dispatcher's limits.  light: the small ones (the SIMT emulator spends seconds on a wide bitmap)."""
    import fuzz_cases as fz
    KK, DENSE = "SPGEMM_KK", "SPGEMM_KK_DENSE"
    cases = []
    add = lambda name, A, B, expect, algo=KK, knobs=None: cases.append((name, A, B, algo, knobs, expect if isinstance(expect, dict) else tuple(expect)))
    L = oracle.laplace3d("FE", 6, 5, 4) if light else oracle.laplace3d("FE", 10, 10, 10)
    add("27-pt squared", L, L, ["wave"])
    quad = quad_rows_cases()
    add("7-pt squared, four rows per wave", quad[0][0], quad[0][1], ["quad"])               # every row at most 32 entries: the rule leaves no other kernel
    add("mixed small and long rows, quad_rows 1", quad[3][0], quad[3][1], ["quad", "wave"])
    add("A P, quad_rows 2", quad[2][0], quad[2][1], ["quad"], knobs={"spgemm_quad_rows": 2})
    add("9-pt squared, quad_rows 0", quad[1][0], quad[1][1], ["wave"], knobs={"spgemm_quad_rows": 0})
    A1 = oracle.random_crs(100, 50, 8, seed=5); B1 = oracle.random_crs(50, 160, 30, seed=6)
    add("duplicate columns in rows of A and of B, unsorted", A1, B1, ["wave"])
    _, _, R, AP = galerkin_operands(8 if light else 12)
    add("Galerkin R (A P)", R, AP, ["quad"])
    Ld = oracle.laplace3d("FE", 5, 4, 3) if light else oracle.laplace3d("FE", 7, 6, 5)
    add("dense accumulator: 27-pt squared", Ld, Ld, ["hbm", "dense_alg"], algo=DENSE)
    add("dense accumulator: hub row of A", hub_matrix(30, 2000, 6, {3: 700}, seed=2), oracle.random_crs(2000, 1500, 10, variance=4, seed=7, sorted_rows=True),
        ["hbm", "dense_alg"], algo=DENSE)
    A, B = limit_operands()
    # 32 lists and 3 | 33, 64 / 65 products, 256 | 128 x 8 | 129 x 8, 256 x 8 | 257, 256 x 8 + 1, 512 | 513, 1024 | 1025, 4096, 4097, 9000 | of which 4097, 9000
    add("rows at the dispatcher's limits", A, B, {"quad": 2, "wave": 4, "win128": 1, "win256": 2, "win512": 3, "win1024": 2, "hub": 4, "hub_multi": 2})
    A0, B0, A1w, B1w, A2w, B2w, _ = dense_row_windows_operands()
    add("A row of 650 entries", A1w, B1w, ["wave", "items_rank"])                           # more than 512 lists and 3 % of the columns: column blocks
    add("A row of 2500 entries", A2w, B2w, ["quad", "items_rank"])
    add("A row of 650 entries, column blocks off", A1w, B1w, ["wave", "win1024"], knobs={"spgemm_block": 0})
    add("A row of 2500 entries, column blocks off", A2w, B2w, ["quad", "hub"], knobs={"spgemm_block": 0})
    Ab, Bb = all_bins_operands()
    add("all bins, B unsorted", Ab, unsorted_rows(Bb), ["wave", "block_small", "block_large", "hbm"])
    Au = oracle.random_crs(60, 150, 20, seed=9); Bu = fz.hubby(np.random.default_rng(12), 150, 9000, 8, 3, 6000, sort=False)
    add("unsorted B with hub rows under duplicate-laden A", Au, Bu, ["hbm"])
    if light:
        return cases
    rng = np.random.default_rng(66)
    Al, Bl = fz.hubby(rng, 8, 4000, 3, 2, 3000), fz.hubby(rng, 4000, 30000, 6, 2, 2000)
    add("long rows of A against hub rows of B", Al, Bl, ["quad", "items_rank", "items_direct"])
    add("long rows of A against hub rows of B, column blocks off", Al, Bl, ["quad", "hub"], knobs={"spgemm_block": 0})
    add("all bins", Ab, Bb, ["wave", "items_rank", "items_direct", "win128"])
    add("hub rows of B", A0, B0, ["items_rank", "items_direct"])
    add("hub rows of B, narrow windows, column blocks off", A0, B0, ["win128"], knobs={"spgemm_win_bits": 4096, "spgemm_val_cap": 192, "spgemm_block": 0})
    add("hub rows of B, force_unsorted", A0, B0, ["hbm"], knobs={"spgemm_force_unsorted": 1})
    A, B = block_kernel_operands()
    for w, items, cap in ((256, 1, 6144), (256, 1, 64), (4096, 1, 1000), (256, 0, 6144), (16384, 1, 6144)):
        add("column blocks w %d items %d cap %d" % (w, items, cap), A, B, ["quad", "blocks_wg"] if not items else (["items_rank", "items_direct"] if cap == 64 else ["items_rank"]),
            knobs={"spgemm_block_w": w, "spgemm_items": items, "spgemm_item_cap": cap})
    A, Bs = val_steps_operands()
    add("lists that overlap heavily", A, Bs[0][1], ["items_rank", "items_direct"])
    add("value windows with several steps (column blocks off)", A, Bs[0][1], ["win128", "win512"], knobs={"spgemm_block": 0})
    A, B = sorted_emission_operands()
    add("entries sorted in LDS", A, B, ["quad", "items_rank", "win128", "win512", "emit_sorted"])
    A, B, Ad, Bd = kept_structure_operands()
    add("kept bitmaps and lists", A, B, ["items_rank", "win128"])
    add("dense rows of C", Ad, Bd, ["items_direct"])
    units, _ = units_operands()
    add("many short lists, units of 4096 columns", units[2][0], units[2][1], ["wave", "items_rank"], knobs={"spgemm_unit_bits": 12})
    add("dense accumulator: random", oracle.random_crs(120, 900, 11, variance=6, seed=4, sorted_rows=True), oracle.random_crs(900, 700, 9, variance=5, seed=6, sorted_rows=True),
        ["hbm", "dense_alg"], algo=DENSE)
    Rm = oracle.rmat(9, 8, seed=7)
    add("R-MAT scale 9 squared", Rm, Rm, ["quad", "wave", "items_rank"])
    return cases


TYPE_GRID = ((np.int32, np.float64), (np.int64, np.float32), (np.int64, np.float64), (np.int32, np.float32))


def check_spgemm_values(be, capfd, mode, value_dtype, light=False, both_offsets=None):
    """every case of exact_cases in one mode and value type (both offset types in mode "signed", the case's number deciding otherwise); the set
    must reach every bin and every value kernel, the dense-accumulator algorithm included.  Mode "cancelling" works on other structures
    ([A A] and B twice), so there the classes are reported and not required.  light: the small cases only, no requirement on the set.
    Prints what it reached (and, in mode "bound", how much of the bound was used) when the last case is through."""
    cov = Coverage(); lines = []; log = lines.append
    if both_offsets is None: both_offsets = mode == "signed" and not light
    for i, (name, A, B, algo, knobs, expect) in enumerate(exact_cases(light)):
        odts = (np.int32, np.int64) if both_offsets else ((np.int32, np.int64)[(i + (value_dtype == np.float32)) % 2],)
        for odt in odts:
            tag = "%s [%s, %s, %s]" % (name, mode, np.dtype(odt).name, np.dtype(value_dtype).name)
            ratio = check_spgemm_exact(be, A, B, mode, odt, value_dtype, algo, knobs, capfd, () if mode == "cancelling" else expect, cov, seed=i, name=tag)
            if mode == "bound": log("%-90s largest error / bound %.3f" % (tag, ratio))
    if mode == "bound":
        log("largest error / bound among the cases that reached each value kernel (%s): %s" % (
            np.dtype(value_dtype).name, ", ".join("%s %.3f" % (k_, v_) for k_, v_ in cov.ratio.items())))
    log("rows per bin: %r\nrows (items) per value kernel: %r" % (cov.bins, cov.kernels))
    print("\n".join(lines))
    if mode != "cancelling" and not light:
        cov.assert_complete("%s, %s" % (mode, np.dtype(value_dtype).name))
    return cov


def check_sort_and_merge_exact(be):
    """sort_and_merge_matrix on exact signed values: sums bit for bit (any order gives the same bits), runs of duplicates that cancel to a
    stored zero, fp32 values, both offset types, graph only (no values)"""
    rng = np.random.default_rng(31)
    lens = [20000, 3, 8193, 0, 700, 1, 40]
    rm = np.zeros(len(lens) + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
    ent = rng.integers(0, 3000, size=rm[-1]).astype(np.int32)                   # about 7 copies of every column in the long row
    for vdt, odt in ((np.float64, np.int32), (np.float32, np.int64)):
        b = value_bits(64, vdt)
        val = exact_values(rng, rm[-1], b)
        for r in (0, 2, 4):                                                        # runs that cancel: every copy of these columns but the last holds v, the last -(count - 1) v
            lo, hi = rm[r], rm[r + 1]
            cols, cnt = np.unique(ent[lo:hi], return_counts=True)
            for c in cols[(cnt >= 2) & (cols % 3 == 0)]:
                at = lo + np.flatnonzero(ent[lo:hi] == c)
                val[at[:-1]] = val[at[0]]
                val[at[-1]] = -(len(at) - 1) * val[at[0]]
        val = val.astype(vdt).astype(np.float64)
        M = oracle.Crs(len(lens), 3000, rm, ent.copy(), val.astype(vdt))
        Cm = kk.sort_and_merge_matrix(dev(be, M, odt))
        r_, e_, v_ = Cm.to_host()
        key = np.repeat(np.arange(len(lens), dtype=np.int64), lens) * 3000 + ent
        order = np.argsort(key, kind="stable")
        first = np.flatnonzero(np.concatenate([[True], key[order][1:] != key[order][:-1]]))
        sums = np.add.reduceat(val.astype(np.longdouble)[order], first)
        grm = np.zeros(len(lens) + 1, dtype=np.int64); np.cumsum(np.bincount(key[order][first] // 3000, minlength=len(lens)), out=grm[1:])
        n = len(first)
        assert np.array_equal(r_.astype(np.int64), grm) and np.array_equal(e_[:n], (key[order][first] % 3000).astype(np.int32))
        assert (sums.astype(np.float64) == sums).all() and (sums == 0).sum() > 100, int((sums == 0).sum())
        assert np.array_equal(v_[:n].astype(np.float64), sums.astype(np.float64)), "sort_and_merge: sums differ from the exact ones"
        G = kk.CrsMatrix.from_host(len(lens), 3000, rm, ent.copy(), None, offset_dtype=odt, backend=be)          # graph only
        Gm = kk.sort_and_merge_matrix(G)
        r_, e_, v_ = Gm.to_host()
        assert v_ is None and np.array_equal(r_.astype(np.int64), grm) and np.array_equal(e_[:n], (key[order][first] % 3000).astype(np.int32))


# --- spmv_struct: the reference's own cases (sparse/unit_test/Test_Sparse_spmv.hpp:609-768, 1096-1104) -----------------
STRUCT_CASES_1D = [(10,)]
STRUCT_CASES_2D = [(25, 21), (20, 25), (22, 22)]
STRUCT_CASES_3D = [(20, 20, 20), (22, 22, 22), (25, 10, 20), (10, 20, 25), (10, 24, 20)]


def struct_matrix(dims, stencil_type):
    if len(dims) == 1:
        return oracle.laplace1d(dims[0])
    name = "FD" if stencil_type == 1 else "FE"
    return oracle.laplace2d(name, *dims) if len(dims) == 2 else oracle.laplace3d(name, *dims)


def check_spmv_struct(be, dims, stencil_type, mode="N", offset_dtype=np.int32, value_dtype=None, vec_dtype=np.float64,
                      seed=13718, A0=None, rank2=False):
    """check_spmv_struct of the reference test (:263-296): alpha/beta in (1,0), (0,1), (1,1) against the oracle's
    restatement of the host path (itself checked against sequential_spmv in test_oracle.py)."""
    A0 = A0 if A0 is not None else struct_matrix(dims, stencil_type)
    rng = np.random.default_rng(seed)
    trans = mode in "TH"
    nin, nout = (A0.nrows, A0.ncols) if trans else (A0.ncols, A0.nrows)
    x = rng.random(nin).astype(vec_dtype); y0 = rng.random(nout).astype(vec_dtype)
    A = dev(be, A0, offset_dtype, value_dtype)
    Ao = A0 if value_dtype is None else oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries,
                                                   A0.values.astype(value_dtype).astype(np.float64))
    max_val = float(np.abs(A0.values).max())
    for alpha, beta in ((1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (-2.5, 0.5)):
        xd, yd = be.from_numpy(x.reshape(-1, 1) if rank2 else x), be.from_numpy(y0.reshape(-1, 1) if rank2 else y0)
        kk.spmv_struct(mode, stencil_type, dims, alpha, A, xd, beta, yd)
        got = be.to_numpy(yd).astype(np.float64).reshape(-1)
        exp = oracle.spmv_struct(mode, stencil_type, dims, Ao, alpha, x.astype(np.float64), beta, y0.astype(np.float64).copy())
        eps_scale = 1.0 if vec_dtype == np.float64 else EPS_F / np.finfo(np.float64).eps
        tol = oracle.spmv_max_error(A0, alpha, beta, max_val=max_val) * eps_scale
        ok, err = fspmv_ok(exp, got, max(tol, 1e-300))
        assert ok, "spmv_struct mismatch dims=%s stencil=%d mode=%s alpha=%g beta=%g: max err %g > tol %g" % (
            dims, stencil_type, mode, alpha, beta, err, tol)
    if not trans:
        # beta == 0 overwrites y: the incoming y (here all NaN) is never read (BLAS convention of the CRS kernels)
        xd = be.from_numpy(x.reshape(-1, 1) if rank2 else x)
        yd = be.from_numpy(np.full(y0.reshape(-1, 1).shape if rank2 else y0.shape, np.nan, dtype=vec_dtype))
        kk.spmv_struct(mode, stencil_type, dims, 1.0, A, xd, 0.0, yd)
        got = be.to_numpy(yd).astype(np.float64).reshape(-1)
        exp = oracle.spmv_struct(mode, stencil_type, dims, Ao, 1.0, x.astype(np.float64), 0.0, np.zeros(nout))
        ok, err = fspmv_ok(exp, got, max(oracle.spmv_max_error(A0, 1.0, 0.0, max_val=max_val) * eps_scale, 1e-300))
        assert ok and np.isfinite(got).all(), "spmv_struct beta=0 must not read y (dims=%s stencil=%d)" % (dims, stencil_type)


def window_code_cases():
    """(name, matrix, window codes expected) for stream_variant 6: column sets that need 1, several, exactly 16 and more
    than 16 windows of 4096 columns per tile, plus a ragged last tile."""
    rng = np.random.default_rng(77)
    out = []
    # multi-diagonal: offsets spread over 7 windows, columns clipped to the matrix
    n, nc = 5000, 400000
    offs = np.array([0, 1, 2, 5000, 5001, 60000, 60007, 130000, 200000, 200001, 300000, 390000])
    cols = (np.arange(n)[:, None] * 2 + offs[None, :])
    keep = cols < nc
    lens = keep.sum(1)
    rm = np.zeros(n + 1, np.int64); rm[1:] = np.cumsum(lens)
    out.append(("diagonals", oracle.Crs(n, nc, rm, cols[keep].astype(np.int32), rng.random(int(rm[-1]))), 1))
    # exactly 16 column clusters per row (16 windows needed), then 17 (falls back to plain entries)
    for k, ok in ((16, 1), (17, 0)):
        n = 1500
        cols = (np.arange(k)[None, :] * 20000 + rng.integers(0, 1000, (n, k))).astype(np.int32)
        cols.sort(axis=1)
        rm = np.arange(n + 1, dtype=np.int64) * k
        out.append(("clusters%d" % k, oracle.Crs(n, 20000 * k, rm, cols.reshape(-1), rng.random(n * k)), ok))
    # uniformly random columns over a wide range: no tile is coverable
    out.append(("random-wide", oracle.random_crs(3000, 3000000, 9, variance=3, seed=5), 0))
    # 27-pt stencil (9 x-lines per tile) with nnz not a multiple of any tile size
    out.append(("27pt", oracle.laplace3d("FE", 24, 19, 13), 1))
    return out


def check_pattern_direct(be, cases=None):
    """Round 6: the row-pattern records straight from the matrix (pat_direct_kernel: rows compared, the window cover over <= 256 column
    intervals per tile) against the records by way of the window codes (pattern_direct 0): the same tiles get a record, y is the same bit
    for bit (same records, same order of the sums), the one tile without a record reads entries instead of codes; 32- and 64-bit offsets,
    both tile sizes, fp32 values.  Matrices with more than one tile in a hundred without a record take the codes either way."""
    took = 0
    for name, A0, npt, _ in (cases or pattern_code_cases()):
        for odt, vdt in ((np.int32, None), (np.int64, np.float32)):
            res = {}
            for direct in (1, 0):
                kn = {"window_codes_min_knnz": 0, "nnz_per_thread": npt, "pattern_codes": 2, "pattern_codes_min_knnz": 0, "pattern_direct": direct}
                rng = np.random.default_rng(5)
                x, y0 = rng.random(A0.ncols), rng.random(A0.nrows)
                A = dev(be, A0, odt, vdt)
                xd, yd = be.from_numpy(x), be.from_numpy(y0)
                h = kk.SPMVHandle("SPMV_DEFAULT")
                for k_, v_ in kn.items(): h.set(k_, v_)
                kk.spmv(h, "N", 1.5, A, xd, 0.5, yd)
                res[direct] = (be.to_numpy(yd).copy(), h.query("pattern_direct"), h.query("pattern_tiles"), h.query("plain_tiles"), h.query("code_tiles"), h.query("tiles"))
                check_spmv(be, A0, "N", 1.5, 0.0, "SPMV_DEFAULT", knobs=kn, max_val=32.0, nans=True, offset_dtype=odt, value_dtype=vdt)
            (y1, d1, p1, pl1, c1, n1), (y0_, d0, p0, pl0, c0, _) = res[1], res[0]
            assert d0 == 0 and np.array_equal(y1, y0_), (name, d1, p1, p0)
            if d1:
                took += 1
                assert p1 == p0 and c1 == 0 and pl1 == n1 - p1 and pl1 <= max(1, n1 // 100), (name, p1, p0, pl1, c1, n1)
            else:
                assert (p1, pl1, c1) == (p0, pl0, c0), (name, res[1][1:], res[0][1:])
    assert took >= 4, took


def pattern_code_cases():
    """(name, matrix, nnz_per_thread, row-pattern records expected) for the staged SpMV kernel's row-pattern codes."""
    out = []
    out.append(("27pt", oracle.laplace3d("FE", 210, 9, 5), 16, True))
    out.append(("27pt-2048", oracle.laplace3d("FE", 120, 11, 5), 8, True))
    out.append(("7pt", oracle.laplace3d("FD", 400, 8, 5), 8, True))
    out.append(("5pt", oracle.laplace2d("FD", 500, 37), 8, True))
    out.append(("3pt", oracle.laplace1d(12000), 16, True))
    # a stencil with a handful of rows carrying one extra explicit zero: more segments in the tiles they fall into
    A0 = oracle.laplace2d("FE", 200, 60)
    rm = A0.row_map.copy(); ent = A0.entries; val = A0.values
    for r in (1234, 1235, 5000, 9000, 9001, 9002, 9003, 9004, 9005, 9006, 9007):       # eight in a row: that tile keeps its codes
        ent = np.insert(ent, rm[r + 1], ent[rm[r + 1] - 1]); val = np.insert(val, rm[r + 1], 0.0); rm[r + 1:] += 1
    out.append(("9pt-perturbed", oracle.Crs(A0.nrows, A0.ncols, rm, ent.astype(np.int32), val), 16, True))
    # Toeplitz band of 40 diagonals (rows longer than a record's table) and a stencil with empty rows: the codes stay
    n = 3000; offs = np.arange(-20, 20)
    cols = np.arange(n)[:, None] + offs[None, :]; keep = (cols >= 0) & (cols < n)
    rm = np.zeros(n + 1, np.int64); rm[1:] = np.cumsum(keep.sum(1))
    out.append(("band40", oracle.Crs(n, n, rm, cols[keep].astype(np.int32), np.random.default_rng(1).random(int(rm[-1]))), 16, False))
    A0 = oracle.laplace2d("FD", 400, 30)
    lens = np.diff(A0.row_map).copy(); keep = np.ones(A0.nnz, bool)
    for r in range(100, A0.nrows, 3000): keep[A0.row_map[r]:A0.row_map[r + 1]] = False; lens[r] = 0
    rm = np.zeros(A0.nrows + 1, np.int64); rm[1:] = np.cumsum(lens)
    out.append(("5pt-empty-rows", oracle.Crs(A0.nrows, A0.ncols, rm, A0.entries[keep], A0.values[keep]), 16, True))
    # banded random columns: staged x, but no two rows share a pattern
    out.append(("banded-random", oracle.random_crs(6000, 6000, 9, variance=0, seed=4, bandwidth=300, sorted_rows=True), 16, False))
    return out


def mixed_tile_cases():
    """(name, matrix) where only SOME tiles of the planned kernel can use the column codes: a stencil with a few rows that
    couple to columns all over the matrix (the rest of the tiles keep codes / staged x / records), and the reverse."""
    rng = np.random.default_rng(21)
    out = []
    A0 = oracle.laplace3d("FE", 40, 30, 12)
    rm = A0.row_map.copy(); ent = A0.entries.copy(); val = A0.values.copy()
    wide = 400000                                            # x is longer than the stencil's grid: the coupling rows reach all over it
    for r in (777, 5000, 5001, 11000):                       # four rows get 40 extra far-apart columns each
        extra = (A0.ncols + np.sort(rng.choice(wide - A0.ncols, size=40, replace=False))).astype(np.int32)
        ent = np.insert(ent, rm[r + 1], extra); val = np.insert(val, rm[r + 1], rng.random(40)); rm[r + 1:] += 40
    out.append(("stencil+dense-rows", oracle.Crs(A0.nrows, wide, rm, ent, val)))
    # first half random wide (no tile coverable), second half a banded block (every tile coverable)
    n = 6000
    top = oracle.random_crs(n // 2, 2000000, 12, variance=0, seed=3)
    band = oracle.random_crs(n // 2, n // 2, 12, variance=0, seed=4, bandwidth=200, sorted_rows=True)       # columns inside [0, 3000)
    rm = np.concatenate([top.row_map, band.row_map[1:] + top.row_map[-1]])
    out.append(("random-then-banded", oracle.Crs(n, 2000000, rm, np.concatenate([top.entries, band.entries]), np.concatenate([top.values, band.values]))))
    return out


def mv4_cases():
    """(name, matrix, rows the plane-marching rank-2 kernel must leave to the gather kernel: None = any, 0 = none) -- lattice
    stencils whose patches, lines and k-chunks are ragged (nx % 32, ny % 4 != 0), boundary rows of a truncated stencil, rows
    that break the pattern"""
    out = [("27pt 40x14x14", oracle.laplace3d("FE", 40, 14, 14), None), ("7pt 35x13x14", oracle.laplace3d("FD", 35, 13, 14), None),
           ("27pt 9x33x17", oracle.laplace3d("FE", 9, 33, 17), None)]
    # clean truncated stencils (every boundary row is a subset whose missing entries point outside): no gather rows.  7 points =
    # the kernel's compiled-in pattern; 19 points (faces + edges) and 11 points = its run-time patterns with 9 and 5 groups
    def truncated(nx, ny, nz, steps, seed):
        i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
        rows, cols = [], []
        for dk, dj, di in steps:
            ok = (i + di >= 0) & (i + di < nx) & (j + dj >= 0) & (j + dj < ny) & (k + dk >= 0) & (k + dk < nz)
            rows.append((k * ny * nx + j * nx + i)[ok]); cols.append(((k + dk) * ny * nx + (j + dj) * nx + i + di)[ok])
        rows = np.concatenate(rows); cols = np.concatenate(cols)
        order = np.lexsort((cols, rows)); rows = rows[order]; cols = cols[order]
        n = nx * ny * nz
        rm = np.zeros(n + 1, dtype=np.int64); np.add.at(rm, rows + 1, 1); rm = np.cumsum(rm)
        return oracle.Crs(n, n, rm, cols.astype(np.int32), np.random.default_rng(seed).random(rows.size) + 0.5)
    seven = ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0))
    nx, ny, nz = 33, 6, 21
    clean = truncated(nx, ny, nz, seven, 12)
    rm, cols, vals, n = clean.row_map, clean.entries, clean.values, clean.nrows
    out.append(("7pt clean 33x6x21", clean, 0))
    nineteen = tuple((dk, dj, di) for dk in (-1, 0, 1) for dj in (-1, 0, 1) for di in (-1, 0, 1) if abs(dk) + abs(dj) + abs(di) <= 2)
    out.append(("19pt clean 20x15x16", truncated(20, 15, 16, nineteen, 13), 0))
    eleven = seven + ((0, -1, -1), (0, 1, 1), (0, -1, 1), (0, 1, -1))
    out.append(("11pt clean 36x9x14", truncated(36, 9, 14, eleven, 14), 0))
    # periodic in i (wrap-around couplings on two faces: those rows cannot conform) and a lattice whose plane stride is a
    # multiple of its line stride only by accident of the sizes (nx = ny)
    per = seven + ((0, 0, 0),)
    def periodic_i(nx, ny, nz, seed):
        i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
        rows, cols = [], []
        for dk, dj, di in seven:
            ii = (i + di) % nx
            ok = (j + dj >= 0) & (j + dj < ny) & (k + dk >= 0) & (k + dk < nz)
            rows.append((k * ny * nx + j * nx + i)[ok]); cols.append(((k + dk) * ny * nx + (j + dj) * nx + ii)[ok])
        rows = np.concatenate(rows); cols = np.concatenate(cols)
        order = np.lexsort((cols, rows)); rows = rows[order]; cols = cols[order]
        n = nx * ny * nz
        rm_ = np.zeros(n + 1, dtype=np.int64); np.add.at(rm_, rows + 1, 1); rm_ = np.cumsum(rm_)
        return oracle.Crs(n, n, rm_, cols.astype(np.int32), np.random.default_rng(seed).random(rows.size) + 0.5)
    out.append(("7pt periodic in i 34x7x20", periodic_i(34, 7, 20, 15), 2 * 7 * 20))
    out.append(("7pt clean 17x17x17", truncated(17, 17, 17, seven, 16), 0))
    # the same with rows that break the pattern: an extra coupling, a dropped interior entry, an emptied row, a wrap-around entry
    rm2 = rm.copy(); ent = cols.astype(np.int32).copy(); val = vals.copy()
    def drop(r, pos):
        nonlocal rm2, ent, val
        at = rm2[r] + pos
        ent = np.delete(ent, at); val = np.delete(val, at); rm2[r + 1:] -= 1
    def add(r, col):
        nonlocal rm2, ent, val
        seg = ent[rm2[r]:rm2[r + 1]]
        at = rm2[r] + int(np.searchsorted(seg, col))
        ent = np.insert(ent, at, col); val = np.insert(val, at, 0.25); rm2[r + 1:] += 1
    mid = (10 * ny + 3) * nx + 17
    drop(mid, 2); add(mid + 1, mid + 9); add(mid + 2 * nx, 5)
    for _ in range(int(rm2[mid + 40 + 1] - rm2[mid + 40])):
        drop(mid + 40, 0)
    out.append(("7pt + broken rows", oracle.Crs(n, n, rm2, ent, val), 4))
    return out


def mv4_duplicate_cases():
    """(name, matrix, plane-marching plan expected, rows it must leave to the gather kernel) -- lattice stencils whose rows store
    a column twice (the reference adds duplicates up: spmv_impl.hpp:240-303 walks entries, not columns).  A pattern row with a
    duplicate would put two values into one slot of the value buffer: such rows are never the pattern and never conform."""
    base = [c for c in mv4_cases() if c[0] == "7pt clean 33x6x21"][0][1]
    def dup_diag(rows_with_dup):
        rm = base.row_map.astype(np.int64); ent = base.entries; val = base.values
        r_of = np.repeat(np.arange(base.nrows), np.diff(rm))
        diag_at = np.flatnonzero(ent == r_of)
        pick = diag_at[rows_with_dup]
        ent2 = np.insert(ent, pick, ent[pick]); val2 = np.insert(val, pick, 0.375 + 0.001 * np.arange(pick.size))
        add = np.zeros(base.nrows + 1, dtype=np.int64); add[np.asarray(rows_with_dup) + 1] = 1
        return oracle.Crs(base.nrows, base.ncols, rm + np.cumsum(add), ent2.astype(np.int32), val2)
    some = np.arange(7, base.nrows, 83)
    return [("7pt, diagonal stored twice in every row", dup_diag(np.arange(base.nrows)), False, 0),
            ("7pt, diagonal stored twice in %d rows" % some.size, dup_diag(some), True, int(some.size))]


def _from_dense_mask(mask, seed, ncols=None):
    """CRS matrix with an entry wherever mask is set (rows ascending), random values in [0.5, 1.5)"""
    n = mask.shape[0]
    rows, cols = np.nonzero(mask)
    rm = np.zeros(n + 1, dtype=np.int64); np.add.at(rm, rows + 1, 1); rm = np.cumsum(rm)
    return oracle.Crs(n, ncols or mask.shape[1], rm, cols.astype(np.int32), np.random.default_rng(seed).random(rows.size) + 0.5)


def block_diagonal(nblocks, bs, seed=0):
    n = nblocks * bs
    rm = np.arange(n + 1, dtype=np.int64) * bs
    ent = (np.repeat(np.arange(nblocks), bs * bs) * bs + np.tile(np.arange(bs), n)).astype(np.int32)
    return oracle.Crs(n, n, rm, ent, np.random.default_rng(seed).random(n * bs) + 0.5)


def multi_dof(A0, ndof, seed=0):
    """every entry of A0 becomes a dense ndof x ndof block (a vector-valued finite-element matrix on A0's mesh)"""
    n = A0.nrows
    lens = np.diff(A0.row_map)
    rm = np.zeros(n * ndof + 1, dtype=np.int64)
    rm[1:] = np.cumsum(np.repeat(lens * ndof, ndof))
    ent = np.empty(int(rm[-1]), dtype=np.int32)
    for r in range(n):
        c = (A0.entries[A0.row_map[r]:A0.row_map[r + 1]].astype(np.int64)[:, None] * ndof + np.arange(ndof)[None, :]).reshape(-1)
        for d in range(ndof):
            ent[rm[r * ndof + d]:rm[r * ndof + d + 1]] = c
    return oracle.Crs(n * ndof, A0.ncols * ndof, rm, ent, np.random.default_rng(seed).random(ent.size) + 0.5)


def mv5_cases():
    """(name, matrix, 16-row tiles the matrix-core rank-2 kernel must describe: None = some, 0 = the kernel must not engage, rows
    it must leave to its gather rows: None = any) under the default thresholds"""
    out = [("block diagonal 32x32", block_diagonal(40, 32, 1), 80, 0),
           ("block diagonal 5x5, 403 rows", _crop_rows(block_diagonal(81, 5, 2), 403), 25, 3),
           ("3 dof on 27-pt 6x5x4", multi_dof(oracle.laplace3d("FE", 6, 5, 4), 3, 3), None, None)]
    n = 500                                                                      # a dense band of 21 diagonals
    ii = np.arange(n)
    out.append(("band of 21 diagonals", _from_dense_mask(np.abs(ii[:, None] - ii[None, :]) <= 10, 4), 31, 4))
    # described tiles first, then rows with columns all over a wide matrix (their tiles fall below the fill threshold)
    top = block_diagonal(20, 16, 5)
    wide = oracle.random_crs(160, 200000, 12, variance=0, seed=6, sorted_rows=True)
    rm = np.concatenate([top.row_map, wide.row_map[1:] + top.row_map[-1]])
    out.append(("blocks then scattered rows", oracle.Crs(480, 200000, rm, np.concatenate([top.entries, wide.entries]), np.concatenate([top.values, wide.values])), 20, 160))
    # tiles the plan cannot describe between tiles it can: a row that descends, a column stored twice, a tile of more than 2048
    # entries, a tile without entries; and a described tile with empty rows inside
    B = block_diagonal(12, 16, 7)
    rm = B.row_map.copy(); ent = B.entries.copy(); val = B.values.copy()
    ent[rm[17]:rm[18]] = ent[rm[17]:rm[18]][::-1]                                 # tile 1: row 17 descends
    ent[rm[35] + 3] = ent[rm[35] + 2]                                             # tile 2: row 35 stores a column twice
    keep = np.ones(ent.size, bool); keep[rm[48]:rm[64]] = False                   # tile 3: no entries at all
    keep[rm[83]:rm[85]] = False                                                   # tile 5: two empty rows inside a described tile
    lens = np.diff(rm); lens[48:64] = 0; lens[83:85] = 0
    rm2 = np.zeros(B.nrows + 1, np.int64); rm2[1:] = np.cumsum(lens)
    out.append(("tiles that cannot be described", oracle.Crs(B.nrows, B.ncols, rm2, ent[keep], val[keep]), 9, 48))
    big = _from_dense_mask(np.ones((32, 150), bool), 8)                           # 16 x 150 = 2400 entries per tile
    out.append(("tiles above 2048 entries", big, 0, None))
    out.append(("uniform random", oracle.random_crs(800, 800, 9, variance=3, seed=5), 0, None))
    return out


def _crop_rows(A0, n):
    e = int(A0.row_map[n])
    return oracle.Crs(n, A0.ncols, A0.row_map[:n + 1].copy(), A0.entries[:e].copy(), A0.values[:e].copy())


def mv3_cases():
    """(name, matrix, staged tiles expected) for the LDS-staged rank-2 kernel"""
    out = [("27pt", oracle.laplace3d("FE", 37, 11, 9), True), ("7pt", oracle.laplace3d("FD", 50, 12, 7), True),
           ("9pt", oracle.laplace2d("FE", 130, 41), True),
           ("banded-random", oracle.random_crs(3000, 3000, 9, variance=4, seed=4, bandwidth=60, sorted_rows=True), True),
           ("random-wide", oracle.random_crs(2000, 50000, 9, variance=3, seed=5), False)]
    name, A0 = mixed_tile_cases()[0]
    out.append((name, A0, True))
    # rows longer than a staged tile may hold, between stencil rows
    A0 = oracle.laplace2d("FD", 90, 40)
    rm = A0.row_map.copy(); ent = A0.entries.copy(); val = A0.values.copy()
    rng = np.random.default_rng(8)
    for r in (500, 2000):
        extra = np.sort(rng.choice(A0.ncols, size=2500, replace=False)).astype(np.int32)
        ent = np.insert(ent, rm[r + 1], extra); val = np.insert(val, rm[r + 1], rng.random(2500)); rm[r + 1:] += 2500
    out.append(("5pt+long-rows", oracle.Crs(A0.nrows, A0.ncols, rm, ent, val), True))
    return out


# ------------------------------------------------------------------------------------------- rank 2: route x type x layout
# (value type, vector type) pairs of the C ABI; a value type of None is fp64
TYPE_PAIRS = ((None, np.float64), (np.float32, np.float64), (np.float32, np.float32))
# (x order, y order, view): contiguous in the four layout pairs, then windows of padded parents (section "views" above)
LAYOUTS = (("C", "C", None), ("F", "F", None), ("C", "F", None), ("F", "C", None), ("C", "C", "even_pitch"), ("C", "C", "odd_start"),
           ("F", "F", "tall"), ("C", "F", "even_pitch"), ("F", "C", "odd_start"), ("C", "F", "tall"), ("F", "C", "even_pitch"))
# (alpha, beta) of the route cells: beta = 0 runs over NaN in Y (alpha = 0 never reaches a kernel: its own cells scale Y)
ALPHA_BETA = ((1.5, 0.0), (-1.0, 0.5), (1.5, -1.0), (-1.0, 0.0))


def _tp_name(vt, yt):
    return "%s/%s" % ("f32" if vt is not None else "f64", "f32" if yt == np.float32 else "f64")


def _mv2_window(A0, nvec):
    """staging window spmv_mv2_kernel compiles for this width and matrix (kk_spmv_mv.hip, KK_MV2)"""
    L = 4 if nvec >= 12 else (2 if nvec >= 3 else 1)
    need = int(1.15 * (64 // L) * A0.nnz / A0.nrows) + 4
    return L, (256 if need <= 256 else (512 if need <= 512 else 1024))


def check_mv_route_matrix(be, light=False, log=None):
    """every rank-2 route x the three (value, vector) type pairs x int32 / int64 offsets x layouts (contiguous C / F, the four pairs,
    windows of padded parents), compared with the float64 oracle, outside cells guarded, the route confirmed by plan queries.
    log: a list the cells are appended to (route, types, offsets, width, layout, what confirmed it).  Returns the set of
    (offset bits, value type, mv4_stencil) that launched the plane-marching kernel."""
    log = [] if log is None else log
    offs = (np.int32, np.int64)
    cyc = [0]

    def layout():
        cyc[0] += 1
        return LAYOUTS[cyc[0] % len(LAYOUTS)]

    def ab():
        return ALPHA_BETA[cyc[0] % len(ALPHA_BETA)]

    def run(route, A0, nvec, vt, yt, off, algo, knobs=None, mode="N", lay=None, max_val=1.0, expect=None, seed=0, ab_=None, x_special=None):
        xo, yo, view = lay or layout()
        alpha, beta = ab_ or ab()
        h = check_spmv_mv(be, A0, nvec, mode, alpha, beta, xo, yo, algo=algo, knobs=knobs, max_val=max_val, nans=(beta == 0.0),
                          offset_dtype=off, value_dtype=vt, vec_dtype=yt, view=view, seed=seed + nvec, x_special=x_special)
        got = {}
        for k_, want in (expect or {}).items():
            got[k_] = h.query(k_)
            ok = want(got[k_]) if callable(want) else got[k_] == want
            assert ok, "%s %s off=%s nvec=%d %s%s view=%s: plan query %s = %r" % (route, _tp_name(vt, yt), np.dtype(off).name, nvec, xo, yo, view,
                                                                                   k_, got[k_])
        log.append((route, _tp_name(vt, yt), np.dtype(off).name, nvec, "%s%s%s" % (xo, yo, "/%s" % (view,) if view else ""), alpha, beta,
                    ", ".join("%s=%d" % kv for kv in got.items()) or "no handle"))
        return h

    f64v = lambda yt: yt == np.float64
    tps = TYPE_PAIRS
    # 1. the handle-less generic kernel: X that is not 16-byte row-major (column-major, odd pitch, odd start); SW 2 / 4 / 8 / 16
    A0 = oracle.random_crs(700 if light else 1500, 650 if light else 1400, 9, variance=4, seed=41)
    for nvec in ((2, 3, 6, 12, 17) if not light else (2, 3, 6, 12)):
        odd_pitch = (2, 1, 2, 1) if nvec % 2 == 0 else (2, 2, 2, 1)
        lays = (("F", "C", None), ("C", "C", "odd_start"), ("C", "F", odd_pitch), ("F", "F", "tall"))
        for ti, (vt, yt) in enumerate(tps):
            for oi, off in enumerate(offs):
                run("generic (no handle)", A0, nvec, vt, yt, off, None, lay=lays[(ti * 2 + oi + nvec) % 4])
    # 2. spmv_mv2_kernel, X row-major (direct) or packed, every lane shape (widths) x staging window (average row length) x NT
    avgs = {1: (3, 6, 12), 2: (5, 10, 20), 4: (9, 20, 40)}
    mats = {a: oracle.random_crs(600 if light else 1200, 1100, a, variance=0, seed=50 + a) for L in avgs for a in avgs[L]}
    seen = set()
    for nvec in ((2, 3, 5, 6, 12, 16, 21, 32) if not light else (2, 3, 6, 12)):
        L = 4 if nvec >= 12 else (2 if nvec >= 3 else 1)
        for wi, a in enumerate(avgs[L]):
            Lw, win = _mv2_window(mats[a], nvec)
            for nt in ((0, 1) if not light else (wi % 2,)):
                for ti, (vt, yt) in enumerate(tps):
                    off = offs[(ti + wi + nt) % 2]
                    direct = (ti + nt) % 2 == 0
                    lay = (("C", "C", None) if nvec % 2 == 0 else ("C", "C", "even_pitch")) if direct else layout()
                    if not direct and lay[0] == "C" and lay[2] in (None, "even_pitch") and nvec % 2 == 0:
                        lay = ("F",) + lay[1:]
                    algo = "SPMV_DEFAULT" if (nvec + wi + ti) % 3 else None
                    if algo is None and not direct:
                        algo = "SPMV_DEFAULT"
                    run("mv2 L%d win%d nt%d %s" % (Lw, win, nt, "direct" if direct else "packed"), mats[a], nvec, vt, yt, off, algo,
                        knobs={"mv_kernel": 2, "mv_nt": nt}, lay=lay,
                        expect=None if algo is None else {"mv4_workgroups": 0, "mv5_tiles": 0, "mv6_chunks": 0, "mv_tiles": 0, "mv_long_rows": 0})
                    seen.add((Lw, win, nt))
    want = {(L, w, nt) for L in (1, 2, 4) for w in (256, 512, 1024) for nt in (0, 1)}
    assert light or seen == want, sorted(want - seen)
    # 3. the long-row kernel (rows above the threshold, a workgroup each) after the gather kernel; Inf in X at the first column of every long
    # row, where the spare slots of a row's last step of 64 entries load from (the lengths are 56, 28, 1 and 16 modulo 64)
    H = hub_matrix(1500, 5000, 6, {5: 3000, 17: 1500, 700: 1025, 1499: 2000, 40: 1024}, seed=3)
    first = {int(H.entries[H.row_map[r]]): np.inf for r in (5, 17, 700, 1499)}
    for ni, nvec in enumerate((2, 5, 16, 17, 33) if not light else (5, 17)):
        for ti, (vt, yt) in enumerate(tps):
            lay3 = layout(); ab3 = ab()
            for xsp in (None, first):                          # finite sums of every long row, then Inf (same layout, alpha, beta)
                run("long rows" + (", Inf in X" if xsp else ""), H, nvec, vt, yt, offs[(ni + ti) % 2], "SPMV_DEFAULT", knobs={"mv6": 0, "mv_long_T": 1024},
                    max_val=50.0, expect={"mv_long_rows": 4, "mv6_chunks": 0}, x_special=xsp, lay=lay3, ab_=ab3)
    # 4. mv3: LDS-staged X tiles (fp64 vectors only: fp32 vectors fall back to the gather kernel with the tile queries at 0)
    M3 = mv3_cases()[0][1]
    for nvec in ((8, 16) if not light else (8,)):
        for ti, (vt, yt) in enumerate(tps):
            for off in (offs if not light else offs[ti % 2:ti % 2 + 1]):
                run("mv3", M3, nvec, vt, yt, off, "SPMV_DEFAULT", knobs={"mv_kernel": 3}, max_val=32.0,
                    expect={"mv_staged_tiles": (lambda v: v > 0) if f64v(yt) else 0, "mv_tiles": (lambda v: v > 0) if f64v(yt) else 0})
    # 5. mv4 on each of its stencil code objects (27-pt, 7-pt, 19-pt = 9 groups, 11-pt = 5 groups), full and partial blocks
    launched = set()
    cases = mv4_cases()
    m4 = [cases[i][1] for i in (0, 1, 4, 5)]
    for mi, M in enumerate(m4):
        for ti, (vt, yt) in enumerate(tps):
            for oi, off in enumerate(offs):
                for nvec in ((5, 16, 21) if not light else ((5,) if (mi + ti + oi) % 2 else (16,))):
                    lay = ("C", "C", "even_pitch") if nvec % 2 else None        # odd widths: the paired stores beside the masked column
                    h = run("mv4", M, nvec, vt, yt, off, "SPMV_DEFAULT", lay=lay, max_val=32.0,
                            expect={"mv4_workgroups": (lambda v: v > 0) if f64v(yt) else 0})
                    if f64v(yt):
                        launched.add((np.dtype(off).itemsize * 8, "f32" if vt is not None else "f64", h.query("mv4_stencil")))
    # 6. mv5 (matrix cores): widths 1 - 5 (the nc = 2 pass), 16, 17, 37; a described block-diagonal matrix, gather rows on another
    B, B2 = mv5_cases()[0][1], mv5_cases()[1][1]
    for ni, nvec in enumerate((1, 2, 3, 4, 5, 16, 17, 37) if not light else (1, 3, 17)):
        for ti, (vt, yt) in enumerate(tps):
            M = B if (ni + ti) % 2 == 0 else B2
            lay = ("C", "C", ("even_pitch", "odd_start")[ti % 2]) if nvec == 1 else None   # width 1 reaches rank 2 only as a strided view
            run("mv5", M, nvec, vt, yt, offs[(ni + ti) % 2], "SPMV_DEFAULT", lay=lay, max_val=1.5,
                expect={"mv5_tiles": (lambda v: v > 0) if f64v(yt) else 0})
    # 7. mv6 (nonzero split), forced
    name, M6 = mv6_cases()[4 if light else 0]
    for ni, nvec in enumerate((1, 2, 5, 16, 33) if not light else (1, 5)):
        for ti, (vt, yt) in enumerate(tps):
            lay = ("C", "C", "even_pitch") if nvec % 2 else None
            run("mv6", M6, nvec, vt, yt, offs[(ni + ti) % 2], "SPMV_DEFAULT", knobs={"mv6": 2}, lay=lay, max_val=50.0,
                expect={"mv6_chunks": -(-M6.nnz // 128) if f64v(yt) else 0})
    # 8. modes T / H: the cached transpose (mode-N dispatch on it) and the atomic kernel (explicit_transpose 0, and no handle)
    T0 = oracle.random_crs(300 if light else 2000, 250 if light else 1600, 9, variance=4, seed=43)
    for ni, nvec in enumerate((1, 3, 16, 17) if not light else (1, 3)):
        for ti, (vt, yt) in enumerate(tps):
            for mi, mode in enumerate("TH"):
                lay = ("C", "C", "odd_start") if nvec == 1 else None
                off = offs[(ni + ti + mi) % 2]
                run("%s cached transpose" % mode, T0, nvec, vt, yt, off, "SPMV_DEFAULT", mode=mode, lay=lay,
                    knobs={"explicit_transpose_min_knnz": 0}, expect={"transpose_cached": 1})
                run("%s atomics" % mode, T0, nvec, vt, yt, off, "SPMV_DEFAULT", mode=mode, lay=lay,
                    knobs={"explicit_transpose": 0}, expect={"transpose_cached": 0})
                if mi == 0:
                    run("T atomics (no handle)", T0, nvec, vt, yt, off, None, mode=mode, lay=lay)
    # 9. alpha = 0: Y scaled by beta (0 over NaN), no kernel of the product; every type pair and layout
    for li, lay in enumerate(LAYOUTS):
        for ti, (vt, yt) in enumerate(tps):
            for beta in (0.0, 0.5):
                run("alpha 0 (scale Y)", A0, (3, 16, 1)[(li + ti) % 3] if lay[2] else (3, 16)[(li + ti) % 2], vt, yt, offs[(li + ti) % 2],
                    "SPMV_DEFAULT" if (li + ti) % 2 else None, lay=lay, ab_=(0.0, beta))
    return launched


def check_strided_rank1(be, light=False):
    """rank-1 x / y as strided views (every k-th element of a padded parent): modes N and T, with and without a handle, on a random
    matrix, a block-diagonal matrix (the matrix-core rank-2 kernel at width 1) and a lattice; a strided x / y for spmv_struct"""
    import pytest
    mats = [("random", oracle.random_crs(700, 640, 9, variance=4, seed=61), 1.0),
            ("block diagonal", block_diagonal(20 if light else 40, 32, 1), 1.5),
            ("27-pt lattice", oracle.laplace3d("FE", 12, 10, 9) if light else mv4_cases()[0][1], 32.0)]
    strides = ((2, 1), (1, 3), (2, 2), (5, 4))
    for mi, (name, A0, mv) in enumerate(mats):
        for si, (xs, ys) in enumerate(strides):
            for mode in "NT":
                for algo in (None, "SPMV_DEFAULT"):
                    vt, yt = TYPE_PAIRS[(mi + si) % 3]
                    alpha, beta = (0.0, 0.5) if si == 3 and mode == "N" and algo is None else ALPHA_BETA[(si + mi + (mode == "T")) % len(ALPHA_BETA)]
                    h = check_spmv(be, A0, mode, alpha, beta, algo, nans=(beta == 0.0), max_val=mv, x_stride=xs, y_stride=ys,
                                   value_dtype=vt, vec_dtype=yt, seed=si)
                    if h is not None and name == "block diagonal" and mode == "N" and yt == np.float64 and alpha != 0.0:
                        assert h.query("mv5_tiles") > 0, (name, xs, ys)
    # spmv_struct: a strided x (and y) takes the unstructured path on the leading numCols / numRows elements of longer vectors
    for dims, stt in (((25, 21), 1), ((10, 12, 9), 2)):
        A0 = struct_matrix(dims, stt)
        for mode in "NT":
            for xs, ys, extra in ((2, 1, 0), (3, 2, 5), (1, 2, 3)):
                rng = np.random.default_rng(xs + 7 * ys)
                nin, nout = (A0.nrows, A0.ncols) if mode == "T" else (A0.ncols, A0.nrows)
                x = rng.random(nin + extra); y0 = rng.random(nout + extra)
                xd, xpd, xp0, xwin = _window_1d(be, x, xs)
                yd, ypd, yp0, ywin = _window_1d(be, y0, ys, fill_bits=SENTINEL_BITS[np.dtype(np.float64)])
                kk.spmv_struct(mode, stt, dims, 1.5, dev(be, A0), xd, 0.5, yd)
                yp = be.to_numpy(ypd)
                assert_outside_unchanged(yp0, yp, ywin, "y")
                assert_outside_unchanged(xp0, be.to_numpy(xpd), slice(0, 0), "x")
                exp = y0.copy()
                exp[:nout] = oracle.spmv_serial(mode, A0, 1.5, x[:nin].copy(), 0.5, y0[:nout].copy())
                ok, err = fspmv_ok(exp, yp[ywin], oracle.spmv_max_error(A0, 1.5, 0.5, max_val=32.0))
                assert ok, ("spmv_struct strided", dims, mode, xs, ys, err)
    # numpy / torch can make views the C ABI cannot take (reversed, broadcast): refused before any work, y untouched
    A0 = mats[0][1]
    A = dev(be, A0)
    y0 = np.full(2 * A0.nrows, 3.0)
    y, one = be.from_numpy(y0), be.from_numpy(np.ones(A0.ncols))
    if be.name == "emu":
        as_strided = np.lib.stride_tricks.as_strided
        bad = ((one[::-1], y[::2]), (as_strided(one, (A0.ncols,), (0,)), y[::2]), (one, as_strided(y, (A0.nrows,), (0,))))
    else:
        bad = ((one[:1].expand(A0.ncols), y[::2]), (one, y[:1].expand(A0.nrows)))
    for xb, yb in bad:
        with pytest.raises(RuntimeError, match="positive strides only"):
            kk.spmv("N", 1.0, A, xb, 0.0, yb)
    assert np.array_equal(be.to_numpy(y), y0)


def check_unsupported_pair_leaves_y(be):
    """an fp64 matrix with fp32 vectors is refused whatever alpha and the matrix are, before Y is touched"""
    import pytest
    for A0 in (oracle.random_crs(50, 40, 4, seed=1), oracle.random_crs(50, 40, 0, seed=1)):
        A = dev(be, A0)
        for alpha in (0.0, 1.0):
            y0 = np.linspace(1.0, 2.0, 50).astype(np.float32)
            y = be.from_numpy(y0)
            with pytest.raises(kk.KkamdError) as ei:
                kk.spmv("N", alpha, A, be.from_numpy(np.ones(40, np.float32)), 0.5, y)
            assert ei.value.status == kk._capi.ERR_UNSUPPORTED
            Y0 = np.ones((50, 3), np.float32)
            Y = _to_dev_2d(be, Y0)
            with pytest.raises(kk.KkamdError) as ei:
                kk.spmv("N", alpha, A, _to_dev_2d(be, np.ones((40, 3), np.float32)), 0.5, Y)
            assert ei.value.status == kk._capi.ERR_UNSUPPORTED
            assert np.array_equal(be.to_numpy(y), y0) and np.array_equal(_to_host_2d(be, Y), Y0)


# ------------------------------------------------------------------------------------------- SpMV: values, exactly
# check_spmv / check_spmv_mv / check_spmv_struct compare with the oracle under the reference's absolute bound (10 eps times the LONGEST row's
# worth of products) on non-negative inputs.  The checks below compare y = beta y0 + alpha op(A) x with a plain numpy reference of their own
# (spmv_by_products, long-double sums of the expanded products): with `==` where the inputs make every partial sum, in any order, exactly
# representable (signed values, sums that cancel, Inf / NaN / stored zeros in x and in A.values, values replaced on a live handle), and within
# the per-entry bound of any order of summation where they do not (mode "bound").  Every case proves its route by plan queries, and a table of
# routes must have been proved from end to end (RouteCoverage).
SPMV_ALPHAS = (1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 3.0)


def spmv_by_products(A0, values, X, mode, alpha, beta, Y0, shortcut=True):
    """Y = beta Y0 + alpha op(A) X by its definition, in np.longdouble, independent of the oracle: every product a(i, j) x(j) expanded, the
    products of an output entry added up, alpha times the sum, then + beta Y0 when beta != 0 (Y0 is not read otherwise).  alpha == 0 or a
    matrix without entries or rows or columns: beta Y0 (zero for beta == 0), whatever A and X hold -- KokkosSparse_spmv.hpp:145.  Rows may be
    unsorted and hold a column several times.  `values` replaces A0.values; X and Y0 rank 1 or rank 2.  0 * Inf and Inf - Inf are NaN by the
    IEEE rules.  shortcut=False: alpha == 0 is no special case (0 * Inf is NaN), as in the reference's spmv_struct, which has no such shortcut.
    Returns (Y, n, S): per output row the number of products n, per entry of Y the sum of |a x| S (both before alpha)."""
    assert np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant, "np.longdouble is no wider than float64 here"
    ld = np.longdouble
    trans = mode in "TH"
    nin, nout = (A0.nrows, A0.ncols) if trans else (A0.ncols, A0.nrows)
    X2 = np.asarray(X, dtype=ld).reshape(nin, -1)
    Y2 = np.asarray(Y0, dtype=ld).reshape(nout, -1)
    k = X2.shape[1]
    row_of = np.repeat(np.arange(A0.nrows, dtype=np.int64), np.diff(A0.row_map))
    out_i, in_i = (A0.entries.astype(np.int64), row_of) if trans else (row_of, A0.entries.astype(np.int64))
    n = np.bincount(out_i, minlength=nout).astype(np.int64) if A0.nnz else np.zeros(nout, dtype=np.int64)
    sums = np.zeros((nout, k), dtype=ld); S = np.zeros((nout, k), dtype=ld)
    with np.errstate(all="ignore"):
        if A0.nnz and nout and nin:
            order = np.argsort(out_i, kind="stable")
            prod = np.asarray(values, dtype=ld)[order, None] * X2[in_i[order]]
            first = np.flatnonzero(np.concatenate([[True], out_i[order][1:] != out_i[order][:-1]]))
            rows = out_i[order][first]
            sums[rows] = np.add.reduceat(prod, first, axis=0)
            S[rows] = np.add.reduceat(np.abs(prod), first, axis=0)
        if (alpha == 0 and shortcut) or A0.nnz == 0 or nout == 0 or nin == 0:
            Y = ld(beta) * Y2 if beta != 0 else np.zeros((nout, k), dtype=ld)
        else:
            Y = ld(alpha) * sums
            if beta != 0:
                Y = Y + ld(beta) * Y2
    shape = np.shape(Y0)
    return Y.reshape(shape), n, S.reshape(shape)


def spmv_n_max(A0, mode):
    """the most products that meet in one entry of y: the longest row (modes N / C), the most-populated column (modes T / H)"""
    if not A0.nnz: return 0
    return int(np.bincount(A0.entries, minlength=A0.ncols).max()) if mode in "TH" else int(np.diff(A0.row_map).max())


def spmv_value_bits(n_max, vec_dtype, value_dtype=None):
    """b: values, x and y0 are signed integers below 2^b times a fixed power of two.  A product has at most 2 b bits, a sum of at most n_max
    of them 2 b + ceil(log2(n_max + 1)); four more bits cover alpha in {+-1, +-2, +-0.5, 3} and the addition of beta y0.  While the total is at
    most P, the precision of the vector type (which the kernels accumulate in), every partial sum in any order, fused or not, is exactly
    representable.  At most 20; fp32 VALUES at most 10 (they must be representable whatever the vector type)."""
    b = min(20, (P_BITS[np.dtype(vec_dtype)] - 4 - int(math.ceil(math.log2(n_max + 1)))) // 2)
    if value_dtype is not None and np.dtype(value_dtype) == np.float32:
        b = min(b, 10)
    return b


def cancelling_values(rng, A0, xr, bc):
    """values for mode "cancelling": xr holds +-2^k only, so v' = -v xr[c] / xr[c'] is exact.  Inside every row the entries pair up,
    v[2i+1] = -v[2i] xr[c(2i)] / xr[c(2i+1)]: each pair adds up to exactly zero from two large terms.  EVEN rows of two or more entries sum
    to exactly 0 (an odd length closes with a triple p - p/2 - p/2); ODD rows keep exactly one product (the unpaired last entry, or a last
    pair p - 2p).  Returns (values, rows whose sum is exactly zero although they hold two or more products)."""
    lens = np.diff(A0.row_map)
    row = np.repeat(np.arange(A0.nrows, dtype=np.int64), lens)
    within = np.arange(A0.nnz, dtype=np.int64) - A0.row_map[:-1][row]
    v = exact_values(rng, A0.nnz, bc)
    ent = A0.entries
    odd = np.flatnonzero(within % 2 == 1)
    v[odd] = -v[odd - 1] * xr[ent[odd - 1]] / xr[ent[odd]]
    rows = np.arange(A0.nrows)
    tri = rows[(rows % 2 == 0) & (lens % 2 == 1) & (lens >= 3)]           # even row, odd length: the last three entries
    a = A0.row_map[tri + 1] - 3
    v[a] *= 2.0
    p = v[a] * xr[ent[a]]
    v[a + 1] = -(p / 2) / xr[ent[a + 1]]; v[a + 2] = -(p / 2) / xr[ent[a + 2]]
    two = rows[(rows % 2 == 1) & (lens % 2 == 0) & (lens >= 2)]           # odd row, even length: the last pair leaves -p
    a = A0.row_map[two + 1] - 2
    v[a + 1] = -2.0 * v[a] * xr[ent[a]] / xr[ent[a + 1]]
    return v, (rows % 2 == 0) & (lens >= 2)


class RouteCoverage:
    """which (route, offset type) of a table a set of cases has PROVED (plan queries held) in which mode, and the largest error / bound seen"""

    def __init__(self, routes):
        self.proved = {r: set() for r in routes}
        self.ratio = {r: 0.0 for r in routes}

    def add(self, route, how, ratio=0.0):
        self.proved[route].add(how)
        self.ratio[route] = max(self.ratio[route], ratio)

    def report(self):
        return "\n".join("%-72s proved in %-12s largest error / bound %.3f" % (" / ".join(r) if isinstance(r, tuple) else r, ",".join(sorted(m)) or "-- nothing --", self.ratio[r]) for r, m in self.proved.items())

    def assert_complete(self, what):
        missing = [r for r, m in self.proved.items() if not m]
        assert not missing, "%s: no case proved the routes %r" % (what, missing)


def _x_targets(A0, mode, rows, extra=()):
    """positions of x that the kernels' clamped loads aim at: column 0, the last column, the first and last column of the longest and of a middle
    row (of `rows`, the rows the route under proof computes), a column no row references, and for modes T / H (x runs over the rows) the x of an
    empty row, the first and the last row"""
    lens = np.diff(A0.row_map)
    cand = np.flatnonzero(lens > 0) if rows is None else np.asarray([r for r in rows if lens[r] > 0])
    longest = int(cand[np.argmax(lens[cand])]); mid = int(cand[len(cand) // 2])
    if mode in "TH":
        pos = [0, A0.nrows - 1, longest, mid]
        empty = np.flatnonzero(lens == 0)
        if empty.size: pos.append(int(empty[empty.size // 2]))
    else:
        pos = [0, A0.ncols - 1]
        for r in (longest, mid):
            pos += [int(A0.entries[A0.row_map[r]]), int(A0.entries[A0.row_map[r + 1] - 1])]
        unused = np.flatnonzero(np.bincount(A0.entries, minlength=A0.ncols) == 0)
        if unused.size: pos.append(int(unused[unused.size // 2]))
    out = []
    for p in list(pos) + [int(e) for e in extra]:
        if p not in out: out.append(p)
    return out


def _classes(Y, rows):
    Yr = np.asarray(Y, dtype=np.float64).reshape(Y.shape[0], -1)
    if rows is not None: Yr = Yr[np.asarray(rows)]
    nan = np.isnan(Yr).any(axis=1); inf = np.isinf(Yr).any(axis=1) & ~nan
    return bool(inf.any()), bool(nan.any()), bool((~nan & ~inf & np.isfinite(Yr).all(axis=1)).any())


def check_spmv_exact(be, A0, how="signed", mode="N", nvec=None, algo=None, knobs=None, proof=None, value_dtype=None, vec_dtype=np.float64,
                     offset_dtype=np.int32, x_order="C", y_order="C", view=None, struct=None, route_rows=None, x_extra=(), zero_at=(),
                     seed=0, name=""):
    """y = beta y0 + alpha op(A) x on the STRUCTURE of A0, with values, x and y0 drawn here, through the same entry points as check_spmv /
    check_spmv_mv / check_spmv_struct (nvec None: rank 1; struct = (stencil_type, dims): spmv_struct), against spmv_by_products.  An analysed
    handle is called a second time when beta == 0; `proof` (a function of the handle's query) must hold afterwards.  By `how`:
      signed      values integers of b bits (spmv_value_bits) times 2^-4, x times 2^-3, y0 times 2^-2, alpha and beta from SPMV_ALPHAS, beta = 0
                  over a y full of NaN: got == expected, entry by entry (signed zeros are not told apart)
      cancelling  (modes N / C) x = +-2^k, entries paired so that even rows sum to exactly 0 from large terms and odd rows keep one product
                  (cancelling_values): `==`, the zero rows are 0 (beta = 0), both parities among the rows the route computes
      special     on signed values: +Inf in x at the positions the clamped loads aim at (_x_targets); then 0, +Inf, -Inf, NaN in turn there;
                  then those four in A.values at special_positions, written in place under a live handle; then finite values written back in
                  place -- handle.values_changed() under values_tracking 1 for 32-bit offsets, exact tracking (the default) for 64-bit ones --
                  and `==` again; then alpha = 0 over the specials in A and x: beta y0 (spmv_struct: beta y0 + 0 * sum, as the reference's, which
                  has no shortcut).  NaN where the expectation is NaN, the same infinity
                  where it is one, `==` elsewhere; every step's expectation holds an Inf row, a NaN row (not the first step: one sign of Inf
                  alone) and a finite row among the rows the route computes
      bound       values uniform in (-50, 50) rounded to the value type, x and y0 in (-1, 1): |got - ref| <= gamma_(n+2) (|alpha| S + |beta y0|)
                  per entry, gamma_m = m u / (1 - m u), u the unit roundoff of the vector type, n and S the entry's products and sum |a x|
                  (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1: n products, n - 1 additions, alpha, beta y0)
    route_rows: the rows the route under proof computes when that is not all of them (the long rows of spmv_mv_long_kernel).  x_extra: more
    positions of x for the special values.  zero_at: positions of A.values that hold a stored 0.0 in every draw and are left out of the
    reference (the entries spmv_struct's interior rows do not read).  Returns (handle, largest error / bound)."""
    vdt = np.dtype(vec_dtype); adt = np.dtype(value_dtype) if value_dtype is not None else np.dtype(np.float64)
    rng = np.random.default_rng([seed, 23])
    trans = mode in "TH"
    assert not (how == "cancelling" and trans)
    nin, nout = (A0.nrows, A0.ncols) if trans else (A0.ncols, A0.nrows)
    k = 1 if nvec is None else nvec
    shape = lambda n_: (n_,) if nvec is None else (n_, nvec)
    zero_at = np.asarray(zero_at, dtype=np.int64)
    keep = np.ones(A0.nnz, dtype=bool); keep[zero_at] = False
    if zero_at.size:                                        # the reference's matrix: A0 without the entries that are never read
        row = np.repeat(np.arange(A0.nrows, dtype=np.int64), np.diff(A0.row_map))[keep]
        rmr = np.zeros(A0.nrows + 1, dtype=np.int64); np.cumsum(np.bincount(row, minlength=A0.nrows), out=rmr[1:])
        Ar = oracle.Crs(A0.nrows, A0.ncols, rmr, A0.entries[keep], np.zeros(int(keep.sum())))
    else:
        Ar = A0
    b = spmv_value_bits(spmv_n_max(Ar, mode), vdt, adt)
    assert b >= 2, "%s: %d products meet in one entry: %d-bit values cannot tell a rounding apart" % (name, spmv_n_max(Ar, mode), b)
    rows_all = route_rows is None
    lens = np.diff(Ar.row_map)

    def full(vr):                                           # values of the library's matrix from those of the reference's
        v = np.zeros(A0.nnz); v[keep] = vr
        return v

    def draw_xy():
        x = (exact_values(rng, nin * k, b) * 2.0).reshape(shape(nin))
        y0 = (exact_values(rng, nout * k, b) * 4.0).reshape(shape(nout))
        return x, y0

    def scalars(i):
        alpha = SPMV_ALPHAS[int(rng.integers(len(SPMV_ALPHAS)))]
        beta = 0.0 if i % 2 == 0 else SPMV_ALPHAS[int(rng.integers(len(SPMV_ALPHAS)))]
        return alpha, beta

    A = dev(be, _with_values(A0, np.zeros(A0.nnz)), offset_dtype, adt)
    h = None
    if algo is not None and struct is None:
        h = kk.SPMVHandle(algo)
        for k_, v_ in (knobs or {}).items(): h.set(k_, v_)
        if how == "special" and offset_dtype == np.int32: h.set("values_tracking", 1)

    def set_values(vr, notify):
        A.values[:] = be.from_numpy(full(vr).astype(adt))
        if notify and h is not None and offset_dtype == np.int32: h.values_changed()

    def call(alpha, beta, x, y0):
        xh = np.asarray(x, order=x_order).astype(vdt, order="K")
        yh = np.full(shape(nout), np.nan, dtype=vdt, order=y_order) if beta == 0.0 else np.asarray(y0, order=y_order).astype(vdt, order="K")
        if nvec is None:
            xd, yd = be.from_numpy(xh), be.from_numpy(yh)
        elif view is not None:
            xd, xpd, xp0, xwin = _window_2d(be, xh, x_order, view_spec(view, nvec, vdt.itemsize))
            yd, ypd, yp0, ywin = _window_2d(be, yh, y_order, view_spec(view, nvec, vdt.itemsize), fill_bits=SENTINEL_BITS[vdt])
        else:
            xd, yd = _to_dev_2d(be, xh), _to_dev_2d(be, yh)
        if struct is not None:
            kk.spmv_struct(mode, struct[0], struct[1], alpha, A, xd, beta, yd)
        elif h is None:
            kk.spmv(mode, alpha, A, xd, beta, yd)
        else:
            kk.spmv(h, mode, alpha, A, xd, beta, yd)
            if beta == 0.0: kk.spmv(h, mode, alpha, A, xd, beta, yd)                   # handle reuse
        if nvec is None:
            return be.to_numpy(yd).astype(np.float64)
        if view is not None:
            Yp = _to_host_2d(be, ypd)
            assert_outside_unchanged(yp0, Yp, ywin, "Y")
            assert_outside_unchanged(xp0, _to_host_2d(be, xpd), (slice(0, 0), slice(0, 0)), "X")
            return Yp[ywin].astype(np.float64)
        return _to_host_2d(be, yd).astype(np.float64)

    def compare(got, Y, n, what):
        with np.errstate(all="ignore"):
            ref = np.asarray(Y, dtype=np.float64)
            fin = np.isfinite(ref)
            assert (ref[fin] == Y[fin]).all() and (ref[fin].astype(vdt).astype(np.float64) == ref[fin]).all(), \
                "%s %s: the reference's sums are not representable in %s (the case's b is wrong)" % (name, what, vdt.name)
        nan = np.isnan(ref)
        bad = (np.isnan(got) != nan) | (~nan & (got != ref))
        if bad.any():
            at = tuple(int(i) for i in np.argwhere(bad)[0])
            raise AssertionError("%s %s: %d entries of y differ, first at %s (%d products): %r, reference %r" % (
                name, what, int(bad.sum()), at, int(n[at[0]]), got[at], ref[at]))

    def representable(*arrs):
        for a_, dt in arrs:
            assert np.array_equal(a_.astype(dt).astype(np.float64), a_, equal_nan=True), name + ": an input is not representable in " + np.dtype(dt).name

    ratio = 0.0
    if how == "signed":
        vr = exact_values(rng, Ar.nnz, b)
        set_values(vr, False)
        for i in range(2):
            x, y0 = draw_xy(); alpha, beta = scalars(i)
            representable((vr, adt), (x, vdt), (y0, vdt))
            Y, n, S = spmv_by_products(Ar, vr, x, mode, alpha, beta, y0)
            compare(call(alpha, beta, x, y0), Y, n, "signed alpha %g beta %g" % (alpha, beta))
    elif how == "cancelling":
        assert b >= 4, "%s: %d-bit values leave nothing after the three bits the pairs cost" % (name, b)
        xr = np.where(rng.random(nin) < 0.5, -1.0, 1.0) * 2.0 ** rng.integers(0, 4, size=nin)
        d = np.where(rng.random(k) < 0.5, -1.0, 1.0) * 2.0 ** rng.integers(0, 2, size=k)       # rank 2: every column of X is xr times +-1 or +-2
        x = xr if nvec is None else np.outer(xr, d)
        vr, zero_rows = cancelling_values(rng, Ar, xr, b - 3)
        sel = np.arange(Ar.nrows) if rows_all else np.asarray(route_rows)
        kept = (sel % 2 == 1) & (lens[sel] >= 1)
        assert zero_rows[sel].any() and kept.any(), "%s: the rows of the route hold %d cancelling and %d product-keeping rows" % (name, int(zero_rows[sel].sum()), int(kept.sum()))
        set_values(vr, False)
        for i in range(2):
            _, y0 = draw_xy(); alpha, beta = scalars(i)
            representable((vr, adt), (x, vdt), (y0, vdt))
            Y, n, S = spmv_by_products(Ar, vr, x, mode, alpha, beta, y0)
            if beta == 0.0:
                Yr = np.asarray(Y, dtype=np.float64).reshape(nout, -1)
                assert (Yr[zero_rows] == 0).all() and (Yr[sel[kept]] != 0).all() and (S.reshape(nout, -1)[zero_rows] > 0).all(), name + ": the cancelling rows do not cancel in the reference"
            got = call(alpha, beta, x, y0)
            compare(got, Y, n, "cancelling alpha %g beta %g" % (alpha, beta))
            if beta == 0.0: assert (got.reshape(nout, -1)[zero_rows] == 0).all()
    elif how == "special":
        vr = exact_values(rng, Ar.nnz, b)
        targets = _x_targets(Ar, mode, route_rows, x_extra)
        hit = np.zeros(nin, dtype=bool); hit[targets] = True
        # a row of the route that meets the fewest targets (at least one) gets positive values there: + Inf and not Inf - Inf
        row_of = np.repeat(np.arange(Ar.nrows, dtype=np.int64), lens)
        if not trans:
            hits = np.bincount(row_of[hit[Ar.entries]], minlength=Ar.nrows)
            cand = np.flatnonzero(hits > 0) if rows_all else np.asarray([r for r in route_rows if hits[r] > 0])
            assert cand.size, name + ": no row of the route references a target column"
            ragged = cand[lens[cand] % 64 != 0]               # a row whose last step of 64 entries (the long-row kernel's) has spare slots, if there is one
            cand = ragged if ragged.size else cand
            r_inf = int(cand[np.argmin(hits[cand])])
            seg = slice(int(Ar.row_map[r_inf]), int(Ar.row_map[r_inf + 1]))
            vr[seg] = np.where(hit[Ar.entries[seg]], np.abs(vr[seg]), vr[seg])
        set_values(vr, False)
        x, y0 = draw_xy()
        sel = None if rows_all else (np.asarray(route_rows) if not trans else None)
        col0 = lambda a_: a_ if nvec is None else a_[:, 0]
        def run(xs, vs, alpha, beta, what, need_nan=True, classes=True, shortcut=True):
            Y, n, S = spmv_by_products(Ar, vs, xs, mode, alpha, beta, y0, shortcut)
            if classes:
                has = _classes(Y, sel)
                assert has[0] and (has[1] or not need_nan) and has[2], "%s %s: the expectation holds (Inf, NaN, finite) rows: %r" % (name, what, has)
            compare(call(alpha, beta, xs, y0), Y, n, what)
        # 1. one sign of Inf in x
        xs = x.copy(); xs[targets] = np.inf
        alpha, beta = scalars(0)
        run(xs, vr, abs(alpha), beta, "special: +Inf in x", need_nan=False)
        # 2. 0, +Inf, -Inf, NaN in turn; the rotation is the first that shows the three classes (found on the reference alone)
        for rot in range(4):
            xs = x.copy()
            xs[targets] = (np.array(SPECIALS)[(np.arange(len(targets)) + rot) % 4])[:, None] if nvec is not None else np.array(SPECIALS)[(np.arange(len(targets)) + rot) % 4]
            if all(_classes(spmv_by_products(Ar, vr, col0(xs), mode, 1.0, 0.0, col0(y0))[0], sel)): break      # (whole rows of X are special: one column tells)
        alpha, beta = scalars(1)
        run(xs, vr, alpha, beta, "special: 0 / Inf / -Inf / NaN in x")
        # 3. the four in A.values, in place under the live handle
        if rows_all or trans:
            pos = special_positions(rng, Ar, extra=min(48, 2 + Ar.nnz // 64))
        else:                                                   # the first entry of three rows of the route (the others stay finite), both ends of a row outside it
            rr = np.asarray(route_rows)[:3]
            other = int(np.flatnonzero((lens > 0) & ~np.isin(np.arange(Ar.nrows), route_rows))[0])
            pos = np.concatenate([Ar.row_map[rr], [Ar.row_map[other], Ar.row_map[other + 1] - 1]])
        for rot in range(4):
            vs = vr.copy(); vs[pos] = np.array(SPECIALS)[(np.arange(len(pos)) + rot) % 4]
            if all(_classes(spmv_by_products(Ar, vs, col0(x), mode, 1.0, 0.0, col0(y0))[0], sel)): break
        set_values(vs, True)
        alpha, beta = scalars(0)
        run(x, vs, alpha, beta, "special: 0 / Inf / -Inf / NaN in A.values")
        # 4. alpha = 0 over specials in A and in x: beta y0 (0 over NaN for beta = 0).  The reference's spmv_struct has no such shortcut (its
        # non-transposed rows compute beta y0 + 0 * sum: NaN where the sum is Inf or NaN), and neither has the library's
        for beta in (0.0, -2.0):
            run(xs, vs, 0.0, beta, "special: alpha 0 over specials", classes=False, shortcut=struct is None or trans)
        # 5. finite values written back in place: nothing non-finite may survive in a copy the plan keeps
        vr2 = exact_values(rng, Ar.nnz, b)
        set_values(vr2, True)
        for i in range(2):
            alpha, beta = scalars(i)
            run(x, vr2, alpha, beta, "special: finite values written back (alpha %g beta %g)" % (alpha, beta), classes=False)
    elif how == "bound":
        vr = rng.uniform(-50, 50, Ar.nnz).astype(adt).astype(np.float64)
        set_values(vr, False)
        u = U_ROUND[vdt]
        for i in range(2):
            x = rng.uniform(-1, 1, shape(nin)).astype(vdt).astype(np.float64); y0 = rng.uniform(-1, 1, shape(nout)).astype(vdt).astype(np.float64)
            alpha, beta = scalars(i)
            Y, n, S = spmv_by_products(Ar, vr, x, mode, alpha, beta, y0)
            got = call(alpha, beta, x, y0)
            m = (n + 2).astype(np.longdouble).reshape((nout,) + (1,) * (got.ndim - 1))
            bound = m * u / (1 - m * u) * (abs(alpha) * S + (np.abs(beta * y0) if beta != 0 else 0))
            err = np.abs(got.astype(np.longdouble) - Y)
            bad = ~(err <= bound)
            if bad.any():
                at = tuple(int(i_) for i_ in np.argwhere(bad)[0])
                raise AssertionError("%s bound alpha %g beta %g: %d entries outside gamma_(n+2) (|alpha| S + |beta y0|), first at %s (%d products): %r, reference %r, bound %g" % (
                    name, alpha, beta, int(bad.sum()), at, int(n[at[0]]), got[at], float(Y[at]), float(bound[at])))
            nz = bound > 0
            if nz.any(): ratio = max(ratio, float((err[nz] / bound[nz]).max()))
    else:
        raise ValueError(how)
    if proof is not None:
        assert h is not None and proof(h.query), "%s: the plan queries do not prove the route: %s" % (name, {k_: h.query(k_) for k_ in (
            "tile", "tiles", "plain_tiles", "code_tiles", "staged_tiles", "pattern_tiles", "pattern_direct", "march_workgroups", "colslab", "colslab_deterministic",
            "transpose_cached", "mv_tiles", "mv_staged_tiles", "mv_long_rows", "mv4_workgroups", "mv4_other_rows", "mv5_tiles", "mv6_chunks")})
    return h, ratio


def plain_tile_matrix(npt, exact, seed=0):
    """rows for the planned kernel's plain tiles of 256 * npt entries: a row of 2 * tile - 100 entries from entry 185 on, which spans three
    tiles (its middle tile holds nothing else: the fixup kernel adds the carries up; 3996 entries at tiles of 2048 still leave fp32 sums
    four bits), rows that end exactly at a tile's end, empty rows, and a last tile that is full (exact) or ragged;
    unsorted rows with duplicate columns"""
    tile = 256 * npt
    lens = [5] * 37 + [2 * tile - 100] + [3, 0, 7] * 40 + [tile - 11] + [1] * 20
    lens.append((-sum(lens)) % tile if exact else ((-sum(lens)) % tile + 13) % tile or 13)
    lens = np.asarray(lens, dtype=np.int64)
    rm = np.zeros(lens.size + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
    assert (rm[-1] % tile == 0) == exact
    rng = np.random.default_rng([seed, npt])
    return oracle.Crs(lens.size, 2 * tile + 77, rm, rng.integers(0, 2 * tile + 77, size=rm[-1]).astype(np.int32), np.ones(rm[-1]))


def values_hub_matrix(seed=3):
    """short rows and hubs whose lengths are 1, 0 and other residues modulo 64 (the long-row kernel walks a row 64 entries at a step), one of
    them exactly at the threshold 1024 (it stays with the gather kernel); columns spread over 30000 so that a long row misses most targets"""
    return hub_matrix(600, 30000, 5, {5: 1089, 17: 1152, 300: 1030, 599: 1100, 40: 1024}, seed=seed)


def struct_extra_entry(dims, stencil_type):
    """(matrix, positions of its extra entries): a stencil matrix whose interior rows r each hold one more entry at their end (a stored 0.0 that
    spmv_struct's interior kernel does not read: the rows of that chunk go through row_map instead of the contiguous block of values)"""
    A0 = struct_matrix(dims, stencil_type)
    rm = A0.row_map.copy(); ent = A0.entries; val = A0.values
    at = []
    for r in (dims[0] + 7, dims[0] + 100):
        at.append(int(rm[r + 1]))
        ent = np.insert(ent, rm[r + 1], ent[rm[r + 1] - 1]); val = np.insert(val, rm[r + 1], 0.0); rm[r + 1:] += 1
    return oracle.Crs(A0.nrows, A0.ncols, rm, ent.astype(np.int32), val), at


F64_PAIRS = ((None, np.float64), (np.float32, np.float64))


def spmv_value_routes(kind, light=False):
    """the table of routes: dicts of name, A0, and what check_spmv_exact takes (algo, knobs, proof, mode, nvec, layouts, struct, ...).
    pairs: the (value, vector) type pairs the route accepts; proof32: the proof when the vectors are fp32 and the route falls back."""
    R = []
    def add(name, A0, algo=None, knobs=None, proof=None, modes="N", pairs=TYPE_PAIRS, **kw):
        R.append(dict(name=name, A0=A0, algo=algo, knobs=knobs, proof=proof, modes=modes, pairs=pairs, kw=kw))
    q_plain = lambda q: q("plain_tiles") == q("tiles") > 0
    only64 = lambda npt: TYPE_PAIRS[:1] if npt == 4 else TYPE_PAIRS           # tiles of 1024 entries exist for fp64 values only
    if kind == "rank1":
        G = oracle.random_crs(300 if light else 1500, 280 if light else 1400, 9, variance=4, seed=41)        # unsorted rows, duplicate columns
        add("vector kernel (no handle)", G, modes="NC")
        for lanes in (1, 4, 64):
            add("vector kernel, FAST_SETUP, %d lanes per row" % lanes, G, "SPMV_FAST_SETUP", {"lanes_per_row": lanes}, lambda q: q("tiles") == 0)
        for npt in (4, 8, 16):
            add("plain tiles of %d, ragged last tile" % (256 * npt), plain_tile_matrix(npt, False), "SPMV_DEFAULT", {"nnz_per_thread": npt},
                lambda q, t=256 * npt: q("tile") == t and q("plain_tiles") == q("tiles") > 3, pairs=only64(npt),
                # a row through three tiles of 4096 holds more than 4095 entries: three bits in fp32 sums, too few for the cancelling pairs
                **({"cancel_pairs": F64_PAIRS} if npt == 16 else {}))
        add("plain tiles of 1024, full last tile", plain_tile_matrix(4, True), "SPMV_DEFAULT", {"nnz_per_thread": 4},
            lambda q: q("tile") == 1024 and q("plain_tiles") == q("tiles") > 3, pairs=only64(4))
        add("code tiles", window_code_cases()[1][1], "SPMV_DEFAULT", {"window_codes_min_knnz": 0, "window_codes": 2, "nnz_per_thread": 8},
            lambda q: q("code_tiles") > 0 and q("staged_tiles") == 0)
        add("staged-x tiles", oracle.laplace3d("FE", 24, 9, 7) if light else oracle.laplace3d("FE", 64, 20, 9), "SPMV_DEFAULT",
            {"window_codes_min_knnz": 0, "nnz_per_thread": 8, "pattern_codes": 0}, lambda q: q("staged_tiles") > 0 and q("pattern_tiles") == 0)
        pcs = {c[0]: c for c in pattern_code_cases()}
        pats = (("one segment (27-pt)", oracle.laplace3d("FE", 60, 9, 5) if light else pcs["27pt"][1], 8 if light else 16),) + \
               (() if light else (("several segments (9-pt, perturbed rows)", pcs["9pt-perturbed"][1], 16), ("several segments (5-pt, empty rows)", pcs["5pt-empty-rows"][1], 16)))
        for what, M, npt in pats:
            # the matrices whose tiles hold several segments leave more than one tile in a hundred without a record: the library builds their
            # records through the codes whatever pattern_direct says (it is asked for here), and the records sit beside tiles that read codes
            several = not what.startswith("one")
            for direct in ((1,) if several else (1, 0)):
                add("pattern tiles, %s, %s" % (what, "through codes, beside code tiles" if several else ("straight from the matrix" if direct else "through codes")),
                    M, "SPMV_DEFAULT", {"window_codes_min_knnz": 0, "nnz_per_thread": npt, "pattern_codes": 2, "pattern_codes_min_knnz": 0, "pattern_direct": direct},
                    (lambda q: q("pattern_tiles") > 0 and q("code_tiles") > 0 and q("pattern_direct") == 0) if several else
                    (lambda q, d=direct: q("pattern_tiles") > 0 and q("pattern_direct") == d), pairs=only64(npt))
        add("mixed tiles", mixed_tile_cases()[1][1], "SPMV_DEFAULT", {"window_codes_min_knnz": 0, "nnz_per_thread": 8, "pattern_codes": 0, "window_codes_min_pct": 10},
            lambda q: 0 < q("plain_tiles") < q("tiles"))
        m4 = {c[0]: c[1] for c in mv4_cases()}
        add("march, every row", m4["7pt clean 33x6x21"], "SPMV_DEFAULT", {"march": 1}, lambda q: q("march_workgroups") > 0 and q("mv4_other_rows") == 0, pairs=F64_PAIRS)
        add("march, with rows left to the gather rows", m4["7pt + broken rows"], "SPMV_DEFAULT", {"march": 1}, lambda q: q("march_workgroups") > 0 and q("mv4_other_rows") == 4, pairs=F64_PAIRS)
        S = oracle.random_crs(700 if light else 3000, 3000, 9, variance=4, seed=3)
        add("column slab, atomic", S, "SPMV_DEFAULT", {"colslab": 2, "colslab_shift": 6}, lambda q: q("colslab") == 1 and q("colslab_deterministic") == 0)
        add("column slab, deterministic", S, "SPMV_DEFAULT", {"colslab": 4, "colslab_shift": 6}, lambda q: q("colslab") == 1 and q("colslab_deterministic") == 1)
        for algo in ("SPMV_MERGE_PATH", "SPMV_NATIVE", "SPMV_NATIVE_MERGE_PATH"):
            add(algo, G, algo, None, q_plain, modes="NC")
        E = mv6_cases()[4][1]                                                                  # empty rows, a row of 1000, 5000 columns
        add("transposed, atomics (no handle)", E, modes="TH")
        add("transposed, atomics (explicit_transpose 0)", E, "SPMV_DEFAULT", {"explicit_transpose": 0}, lambda q: q("transpose_cached") == 0, modes="TH")
        add("transposed, cached transpose", E, "SPMV_DEFAULT", {"explicit_transpose": 1, "explicit_transpose_min_knnz": 0}, lambda q: q("transpose_cached") == 1, modes="TH")
    elif kind == "struct":
        # grids with two or three chunks of interior rows per line; specials on boundary points (_x_targets: the first and the last column) and
        # on the halo of an interior chunk: the points left and right of the chunk that begins at i = 65
        for what, dims, st in (("1-D", (300,), 1), ("2-D FD", (140, 6), 1), ("2-D FE", (140, 6), 2), ("3-D FD", (140, 5, 4), 1), ("3-D FE", (140, 5, 4), 2)):
            line = 0 if len(dims) == 1 else (dims[0] * (2 if len(dims) == 2 else dims[1] + 2))
            add("spmv_struct %s" % what, struct_matrix(dims, st), struct=(st, dims), x_extra=(line + 64, line + 129), modes="NT" if what == "2-D FE" else "N")
        A1, at = struct_extra_entry((140, 6), 2)
        add("spmv_struct 2-D FE, rows with an extra entry", A1, struct=(2, (140, 6)), zero_at=at, x_extra=(2 * 140 + 64, 2 * 140 + 129))
    elif kind == "rank2":
        G = oracle.random_crs(300 if light else 1500, 280 if light else 1400, 9, variance=4, seed=41)
        add("generic (no handle)", G, nvecs=(3, 12), lays=(("F", "C", None), ("C", "C", "odd_start"), ("F", "F", "tall")), modes="NC")
        M2 = oracle.random_crs(300 if light else 1200, 1100, 10, variance=0, seed=60)
        none = lambda q: q("mv4_workgroups") == 0 and q("mv5_tiles") == 0 and q("mv6_chunks") == 0 and q("mv_tiles") == 0 and q("mv_long_rows") == 0
        for nt in (0, 1):
            add("gather kernel, nt %d" % nt, M2, "SPMV_DEFAULT", {"mv_kernel": 2, "mv_nt": nt}, none, nvecs=(2, 5, 16), lays=(("C", "C", None), ("F", "F", None), ("C", "F", "even_pitch")))
        H = values_hub_matrix()
        long_rows = [int(r) for r in np.flatnonzero(np.diff(H.row_map) > 1024)]
        add("long rows", H, "SPMV_DEFAULT", {"mv6": 0, "mv_long_T": 1024}, lambda q: q("mv_long_rows") == 4 and q("mv6_chunks") == 0, nvecs=(5, 16, 17),
            lays=(("C", "C", None), ("F", "F", None), ("C", "F", None)), route_rows=long_rows)
        add("mv3 (LDS-staged X)", oracle.laplace3d("FE", 20, 9, 7) if light else mv3_cases()[0][1], "SPMV_DEFAULT", {"mv_kernel": 3},
            lambda q: q("mv_staged_tiles") > 0 and q("mv_tiles") > 0, proof32=lambda q: q("mv_staged_tiles") == 0 and q("mv_tiles") == 0, nvecs=(8, 16))
        cases = mv4_cases()
        for i in ((0,) if light else (0, 1, 4, 5)):
            add("mv4 (plane marching) on %s" % cases[i][0], cases[i][1], "SPMV_DEFAULT", None, lambda q: q("mv4_workgroups") > 0, proof32=lambda q: q("mv4_workgroups") == 0,
                nvecs=(5, 16), lays=(("C", "C", "even_pitch"), ("F", "F", None)))
        five = mv5_cases()
        for i in ((0,) if light else (0, 1)):
            add("mv5 (matrix cores) on %s" % five[i][0], five[i][1], "SPMV_DEFAULT", None, lambda q: q("mv5_tiles") > 0, proof32=lambda q: q("mv5_tiles") == 0, nvecs=(3, 16, 17))
        E = mv6_cases()[4][1]
        add("mv6 (nonzero split)", E, "SPMV_DEFAULT", {"mv6": 2}, lambda q, c=-(-E.nnz // 128): q("mv6_chunks") == c, proof32=lambda q: q("mv6_chunks") == 0, nvecs=(2, 5, 16),
            lays=(("C", "C", "even_pitch"), ("F", "F", None), ("C", "C", None)))
        T0 = oracle.random_crs(300 if light else 2000, 250 if light else 1600, 9, variance=4, seed=43)
        add("transposed, atomics (no handle)", T0, nvecs=(3, 16), modes="TH")
        add("transposed, atomics (explicit_transpose 0)", T0, "SPMV_DEFAULT", {"explicit_transpose": 0}, lambda q: q("transpose_cached") == 0, nvecs=(3, 16), modes="TH")
        add("transposed, cached transpose", T0, "SPMV_DEFAULT", {"explicit_transpose_min_knnz": 0}, lambda q: q("transpose_cached") == 1, nvecs=(3, 17), modes="TH")
    else:
        raise ValueError(kind)
    return R


VALUE_MODES = ("signed", "cancelling", "special", "bound")


def check_spmv_values(be, how, kind, light=False, offsets=(np.int32, np.int64)):
    """every route of spmv_value_routes(kind) in mode `how`: for each offset type of `offsets`, EVERY (value, vector) type pair the route accepts
    (their kernels are separate instantiations), widths, layouts and transposition modes taking turns with the call, the offset type and the mode
    (so that the four modes and two offset types between them walk every width of the table on every pair).  The route is proved by its plan
    queries at every call, and at the end every route must have been proved with every offset type asked for (mode "cancelling" has no
    transposed form: those routes are left out of its table).  light: one call per route, offset types and type pairs in turn, every route
    proved once.  A pair that leaves too few bits for the values (spmv_value_bits below 2; below 4 in mode "cancelling", whose pairs cost
    three) is an error in the table: a route says which pairs it takes in mode "cancelling" where those are fewer (cancel_pairs).
    A call without a handle and spmv_struct have no plan to query: what they run follows from the call alone (no analysis, a matrix below
    transient_min_knnz: the vector kernel, the atomic transposed kernel, the generic rank-2 kernel; the structured kernels).  A rank-2 route
    whose kernel takes fp64 vectors only is called with fp32 vectors too, must say so in its queries (proof32), and that call does not count
    as proof.  Prints what was proved and, in mode "bound", the largest error / bound per route."""
    routes = [r for r in spmv_value_routes(kind, light) if not (how == "cancelling" and r["modes"] == "TH")]
    onames = ["any"] if light else [np.dtype(o).name for o in offsets]
    cov = RouteCoverage([(r["name"], o) for r in routes for o in onames])
    need = 4 if how == "cancelling" else 2
    hk = VALUE_MODES.index(how)
    for ri, r in enumerate(routes):
        kw = dict(r["kw"])
        nvecs = kw.pop("nvecs", (None,)); lays = kw.pop("lays", (("C", "C", None), ("F", "F", None))); proof32 = kw.pop("proof32", None)
        cancel_pairs = kw.pop("cancel_pairs", None)
        modes = "N" if how == "cancelling" and r["modes"] == "NT" else r["modes"]
        pairs = list(cancel_pairs if how == "cancelling" and cancel_pairs is not None else r["pairs"])
        for vt, yt in pairs:
            bits = min(spmv_value_bits(spmv_n_max(r["A0"], m_), yt, vt) for m_ in modes)
            assert bits >= need, "%s: %s leaves %d bits for the values, mode %s needs %d" % (r["name"], _tp_name(vt, yt), bits, how, need)
        proving = [p_ for p_ in pairs if not (proof32 is not None and nvecs[0] is not None and p_[1] == np.float32)]
        if light:
            calls = [((np.int32, np.int64)[(ri + hk) % 2], proving[(ri + hk) % len(proving)])]
        else:
            calls = [(off, p_) for off in offsets for p_ in pairs]
        for ci, (off, (vt, yt)) in enumerate(calls):
            i = ri + ci + hk + (np.dtype(off).itemsize // 8)
            nvec = nvecs[i % len(nvecs)]
            xo, yo, view = lays[(i + i // len(nvecs)) % len(lays)] if nvec is not None else ("C", "C", None)
            mode = modes[i % len(modes)]
            fallback = (vt, yt) not in proving
            proof = proof32 if fallback else r["proof"]
            tag = "%s [%s, %s, %s, mode %s%s]" % (r["name"], how, np.dtype(off).name, _tp_name(vt, yt), mode, "" if nvec is None else ", %d columns %s%s %s" % (nvec, xo, yo, view or ""))
            h, ratio = check_spmv_exact(be, r["A0"], how, mode, nvec, r["algo"], r["knobs"], proof, vt, yt, off, xo, yo, view, seed=i, name=tag, **kw)
            if not fallback:
                cov.add((r["name"], "any" if light else np.dtype(off).name), how, ratio)
    print("SpMV values, %s, %s:\n%s" % (kind, how, cov.report()))
    cov.assert_complete("%s, %s" % (kind, how))
    return cov
