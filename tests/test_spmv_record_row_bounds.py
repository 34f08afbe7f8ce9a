"""Pattern tiles of the planned rank-1 kernel (kk_spmv.hip, spmv_stream3_kernel) take every row boundary from their record and read no row_map:
virtual row j of segment g (first virtual row q_g, in the record) holds the tile's nonzeros [(j - q_g) L_g - jadd_g, + L_g), clamped to the tile;
one-segment tiles and tiles of up to four segments select with constants in scalar registers, tiles of five to eight segments read their
segment's constants from the record in LDS, and tiles with more virtual rows than row groups take the bounds of their later passes from the
record in memory (pat_row_bounds).  The arithmetic is integer and exact, so nothing changes a value.

The cases are the five grids of test_spmv_scalar_chunks.py (one segment; 2-4 segments at both tile sizes; 5-8 segments next to code tiles, whose
bounds still come from row_map; a thin grid), the smallest 27-point grid found by search whose tiles all have records and in which a tile
boundary leaves a single entry of a row behind it, and a 7-point grid with 307 to 409 rows per 2048-nonzero tile: two passes over 256 row
groups.  Tile boundaries that coincide with a row boundary, and boundaries that leave a single entry of the cut row on one side, are counted on
the host (test_boundary_kinds): they are where a clamp of the record's bounds can go wrong.  Each case runs the reference's comparator, the
exact-value checks, Inf / NaN in A.values on both sides of tile ends, and a bit-for-bit comparison with the same handle without pattern records
(row_map-driven bounds).  One body, two backends: the SIMT emulator (no GPU) and the gfx950 library (`-m gpu`)."""
import numpy as np
import pytest

import oracle
import parity_cases as pc


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def be(request):
    if request.param == "emu":
        from emu import emu_backend
        return emu_backend.backend()
    import ctypes as C
    b = pc.kk.torch_backend()
    name = C.create_string_buffer(256); g = C.c_int(); cus = C.c_int()
    pc.kk._capi.check(b.lib, b.lib.kkamd_device_info(name, 256, C.byref(g), C.byref(cus)))
    assert g.value == 1, "libkkamd.so is built for gfx950 only; found %s" % name.value.decode()
    return b


# (id, stencil, grid, nnz_per_thread, tiles, pattern tiles, plain tiles, code tiles)
CASES = [
    ("one-segment", "FE", (400, 4, 3), 16, 21, 20, 1, 0),       # one-segment tiles; ragged plain last tile
    ("2-4-segments", "FE", (160, 6, 4), 16, 19, 18, 1, 0),
    ("2-4-segments-2048", "FE", (80, 9, 5), 8, 38, 37, 1, 0),
    ("5-8-segments", "FE", (80, 9, 5), 16, 19, 11, 0, 8),       # pattern and code tiles interleave
    ("few-chunks", "FE", (72, 3, 4), 8, 8, 7, 1, 0),
    ("one-behind", "FE", (52, 3, 5), 8, 7, 6, 1, 0),            # two boundaries with one entry of the cut row behind them
    ("two-passes", "FD", (400, 3, 3), 8, 10, 9, 1, 0),          # 7-point: more than 256 virtual rows in every full tile
]
IDS = [c[0] for c in CASES]

_MATRICES = {}


def _matrix(case):
    key = (case[1], case[2])
    if key not in _MATRICES:
        _MATRICES[key] = oracle.laplace3d(case[1], *case[2])
    return _MATRICES[key]


def _knobs(npt, pattern_codes=2):
    return {"window_codes_min_knnz": 0, "nnz_per_thread": npt, "pattern_codes": pattern_codes}


def _boundaries(A0, tile):
    """interior tile boundaries p = b * tile < nnz, and by kind: on a row boundary; inside a row (the row is cut: it starts in tile b - 1, since no
    row of these matrices is longer than a tile); cut with one entry in front; cut with one entry behind"""
    p = np.arange(tile, A0.nnz, tile, dtype=np.int64)
    rm = np.asarray(A0.row_map, dtype=np.int64)
    on = np.isin(p, rm)
    return p, on, ~on, ~on & np.isin(p - 1, rm), ~on & np.isin(p + 1, rm)


def test_boundary_kinds():
    # among the cases: a tile boundary on a row boundary, a cut row with a single entry in front of the boundary and one with a single entry
    # behind it; and the two-pass case really has more virtual rows than row groups
    kinds = np.zeros(3, dtype=np.int64)
    for case in CASES:
        A0 = _matrix(case)
        tile = 256 * case[3]
        p, on, cut, one_front, one_behind = _boundaries(A0, tile)
        assert p.size == case[4] - 1
        kinds += (int(on.sum()), int(one_front.sum()), int(one_behind.sum()))
        if case[0] == "two-passes":
            starts = np.bincount(np.asarray(A0.row_map[:-1]) // tile, minlength=case[4])
            assert starts[:-1].min() > 256, starts
    assert (kinds > 0).all(), kinds


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parity_and_tile_counts(be, case):
    name, _, _, npt, tiles, pat, plain, code = case
    A0 = _matrix(case)
    for odt, vdt in ((np.int32, None), (np.int64, np.float32)):
        h = pc.check_spmv(be, A0, "N", 1.5, 0.5, "SPMV_DEFAULT", knobs=_knobs(npt), max_val=32.0, offset_dtype=odt, value_dtype=vdt)
        got = tuple(h.query(k) for k in ("tiles", "pattern_tiles", "plain_tiles", "code_tiles"))
        assert got == (tiles, pat, plain, code), (name, got)
        pc.check_spmv(be, A0, "N", 1.0, 0.0, "SPMV_DEFAULT", nans=True, knobs=_knobs(npt), max_val=32.0, offset_dtype=odt, value_dtype=vdt)


@pytest.mark.parametrize("how", ["signed", "special"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_values(be, case, how):
    pc.check_spmv_exact(be, _matrix(case), how, algo="SPMV_DEFAULT", knobs=_knobs(case[3]), proof=lambda q: q("pattern_tiles") > 0, name=case[0])


def _both_routes(be, A0, npt, values, x, y0, alpha, beta):
    """y of the pattern route and of the same handle type without records"""
    A = pc.dev(be, oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, values))
    ys = {}
    for pat in (2, 0):
        h = pc.kk.SPMVHandle("SPMV_DEFAULT")
        for k_, v_ in _knobs(npt, pat).items(): h.set(k_, v_)
        yd = be.from_numpy(y0.copy())
        pc.kk.spmv(h, "N", alpha, A, be.from_numpy(x), beta, yd)
        ys[pat] = be.to_numpy(yd).copy()
        assert (h.query("pattern_tiles") > 0) == (pat == 2), (pat, h.query("pattern_tiles"))
    return ys


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_same_bits_as_without_records(be, case):
    # both routes multiply the same values and add them in the same order: y with row bounds from the records == y with row bounds from row_map
    A0 = _matrix(case)
    rng = np.random.default_rng(13)
    ys = _both_routes(be, A0, case[3], rng.random(A0.nnz) - 0.5, rng.random(A0.ncols), rng.random(A0.nrows), 1.5, 0.5)
    assert np.array_equal(ys[2], ys[0]), (case[0], int((ys[2] != ys[0]).sum()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_specials_at_tile_ends(be, case):
    # Inf / NaN in A.values next to tile ends: the first entry behind a tile, the last entry of a cut row, the first entry of the row behind a
    # cut row, the last entry in front of a tile end, and the matrix's last entry.  A bound that is off by one moves a special value into a
    # neighbouring row.  The expectation is the class of every row (NaN / +Inf / -Inf / finite) from the products, and the bits of the route
    # without records.
    name, npt = case[0], case[3]
    A0 = _matrix(case)
    tile = 256 * npt
    rm = np.asarray(A0.row_map, dtype=np.int64)
    rng = np.random.default_rng(17)
    values = rng.integers(1, 8, A0.nnz).astype(np.float64)
    x = rng.integers(1, 8, A0.ncols).astype(np.float64)
    y0 = rng.integers(1, 8, A0.nrows).astype(np.float64)
    p, _, cut, _, _ = _boundaries(A0, tile)
    assert cut.sum() >= 2, name
    cp = p[cut][np.arange(4) % int(cut.sum())]
    row_end = rm[np.searchsorted(rm, cp, side="right")]            # end of the row each boundary cuts
    pos = {int(cp[0]): np.inf, int(row_end[1] - 1): np.nan, int(row_end[2]): -np.inf, int(cp[3] - 1): np.nan, A0.nnz - 1: np.inf}
    for i, v in pos.items(): values[i] = v
    ys = _both_routes(be, A0, npt, values, x, y0, 2.0, 0.5)
    rows = np.repeat(np.arange(A0.nrows), np.diff(rm))
    prod = values * x[A0.entries]
    nan = np.bincount(rows, np.isnan(prod), A0.nrows) > 0
    pinf = np.bincount(rows, prod == np.inf, A0.nrows) > 0
    ninf = np.bincount(rows, prod == -np.inf, A0.nrows) > 0
    nan |= pinf & ninf
    got = ys[2]
    assert np.array_equal(np.isnan(got), nan), (name, np.flatnonzero(np.isnan(got) != nan)[:8])
    assert np.array_equal(got == np.inf, pinf & ~nan) and np.array_equal(got == -np.inf, ninf & ~nan), name
    assert nan.any() and (pinf & ~nan).any() and np.isfinite(got).any(), name
    assert np.array_equal(ys[2], ys[0], equal_nan=True), (name, int(((ys[2] != ys[0]) & ~(np.isnan(ys[2]) & np.isnan(ys[0]))).sum()))
