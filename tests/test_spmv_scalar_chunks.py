"""Pattern tiles of the planned rank-1 kernel (kk_spmv.hip, spmv_stream3_kernel) take the first columns of their x chunks from scalar registers: wave
w stages the chunks 8 w ... 8 w + 7 of the tile's window, their columns read with one scalar load and the chunks requested in front of the value
stream, and the launch reads no tile list where the pattern tiles are tiles 0 ... n - 1 (plan query "pattern_list_identity").  None of that changes
a value.  The cases are the four grids of test_spmv_tile_issue_order.py (one-segment tiles and a ragged last tile, 2-4 segments at both tile sizes,
5-8 segments beside code tiles; 4800 and 3840 columns, multiples of 64, and 3600, which is none) and a thin grid whose first and last pattern tiles
need 7 chunks, so that waves 1-3 load nothing but clamped chunks and write none; the one-segment grid has tiles of more than 24 chunks, so that wave
3 writes.  Each case runs the reference's comparator, the exact-value checks (signed values; Inf / NaN at the positions clamped loads aim at) and a
bit-for-bit comparison with the same handle without pattern records.  One body, two backends: the SIMT emulator (no GPU) and the gfx950 library
(`-m gpu`).

The tile counts, the tile modes and the chunk counts are properties of the plan and of the matrix (they hold before and after the kernel's change);
they prove that a case reaches the tiles it is here for."""
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


# (id, grid of the 27-point FE Laplacian, nnz_per_thread, tiles, pattern tiles, plain tiles, code tiles)
CASES = [
    ("one-segment", (400, 4, 3), 16, 21, 20, 1, 0),             # one-segment tiles; ragged last tile; tiles of 22 to 28 chunks
    ("2-4-segments", (160, 6, 4), 16, 19, 18, 1, 0),            # at most one line end per tile
    ("2-4-segments-2048", (80, 9, 5), 8, 38, 37, 1, 0),         # the same at the 2048 tile
    ("5-8-segments", (80, 9, 5), 16, 19, 11, 0, 8),             # two line ends per tile, next to tiles that keep their codes
    ("few-chunks", (72, 3, 4), 8, 8, 7, 1, 0),                  # 216 columns to a plane: seven full tiles of 7 to 11 chunks
]
IDS = [c[0] for c in CASES]

_MATRICES = {}


def _matrix(dims):
    if dims not in _MATRICES:
        _MATRICES[dims] = oracle.laplace3d("FE", *dims)
    return _MATRICES[dims]


def _knobs(npt, pattern_codes=2):
    return {"window_codes_min_knnz": 0, "nnz_per_thread": npt, "pattern_codes": pattern_codes}


def _chunks(cols):
    """64-column chunks of x the analysis stages for a tile with these columns (pat_direct_kernel / win_build_kernel): a window begins at the lowest
    column not yet covered and takes chunks of 64 columns until the first one that holds no column of the tile"""
    c = np.unique(cols)
    n = i = 0
    while i < c.size:
        base, k = int(c[i]), 0
        while k < 64 and np.searchsorted(c, base + 64 * k) < np.searchsorted(c, base + 64 * k + 64):
            k += 1
        n += k
        i = int(np.searchsorted(c, base + 64 * k))
    return n


def _planned(be, case):
    """a handle that has run the case once, its tile modes and the chunks every full tile needs"""
    _, dims, npt = case[:3]
    A0 = _matrix(dims)
    h = pc.check_spmv(be, A0, "N", 1.5, 0.5, "SPMV_DEFAULT", knobs=_knobs(npt), max_val=32.0)
    tile = 256 * npt
    assert h.query("tile") == tile
    modes = h.export("tile_mode", h.query("tiles")) & 3
    chunks = np.array([_chunks(A0.entries[b * tile:(b + 1) * tile]) for b in range(A0.nnz // tile)])
    return h, modes, chunks


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parity_and_tile_counts(be, case):
    _, dims, npt, tiles, pat, plain, code = case
    A0 = _matrix(dims)
    for odt, vdt in ((np.int32, None), (np.int64, np.float32)):
        h = pc.check_spmv(be, A0, "N", 1.5, 0.5, "SPMV_DEFAULT", knobs=_knobs(npt), max_val=32.0, offset_dtype=odt, value_dtype=vdt)
        got = tuple(h.query(k) for k in ("tiles", "pattern_tiles", "plain_tiles", "code_tiles"))
        assert got == (tiles, pat, plain, code), (case[0], got)
        pc.check_spmv(be, A0, "N", 1.0, 0.0, "SPMV_DEFAULT", nans=True, knobs=_knobs(npt), max_val=32.0, offset_dtype=odt, value_dtype=vdt)


@pytest.mark.parametrize("how", ["signed", "special"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_values(be, case, how):
    name, dims, npt = case[:3]
    pc.check_spmv_exact(be, _matrix(dims), how, algo="SPMV_DEFAULT", knobs=_knobs(npt), proof=lambda q: q("pattern_tiles") > 0, name=name)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_same_bits_as_without_records(be, case):
    # both routes multiply the same values and add them in the same order: y with pattern records == y with the window codes
    name, dims, npt = case[:3]
    A0 = _matrix(dims)
    rng = np.random.default_rng(11)
    x, y0 = rng.random(A0.ncols), rng.random(A0.nrows)
    A = pc.dev(be, A0)
    ys = {}
    for pat in (2, 0):
        h = pc.kk.SPMVHandle("SPMV_DEFAULT")
        for k_, v_ in _knobs(npt, pat).items(): h.set(k_, v_)
        yd = be.from_numpy(y0.copy())
        pc.kk.spmv(h, "N", 1.5, A, be.from_numpy(x), 0.5, yd)
        ys[pat] = be.to_numpy(yd).copy()
        assert (h.query("pattern_tiles") > 0) == (pat == 2), (name, pat, h.query("pattern_tiles"))
    assert np.array_equal(ys[2], ys[0]), (name, int((ys[2] != ys[0]).sum()))


def test_chunks_per_tile(be):
    # a wave stages eight consecutive chunks: a pattern tile of fewer than 8 leaves waves 1-3 with clamped, unwritten chunks alone; one of more
    # than 24 makes wave 3 write.  Every pattern tile fits the 32 chunks of the window.
    by_id = {c[0]: c for c in CASES}
    h, modes, chunks = _planned(be, by_id["few-chunks"])
    assert chunks.size >= 4, chunks
    few = chunks[modes[:chunks.size] == 3]
    assert few.size and few.min() < 8, (modes, chunks)
    h, modes, chunks = _planned(be, by_id["one-segment"])
    many = chunks[modes[:chunks.size] == 3]
    assert many.size and 24 < many.max() <= 32, (modes, chunks)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_list_paths(be, case):
    # the launch of the pattern tiles reads no tile list exactly where they are the tiles 0 ... pattern_tiles - 1; both paths are among the cases:
    # the one-segment grid (every tile but the ragged last one) and the 5-8-segment grid, where pattern and code tiles interleave
    h, modes, _ = _planned(be, case)
    pat = h.query("pattern_tiles")
    assert pat == int((modes == 3).sum())
    identity = int(pat > 0 and bool((modes[:pat] == 3).all()))
    assert h.query("pattern_list_identity") == identity, (case[0], modes)
    if case[0] in ("one-segment", "5-8-segments"):
        assert identity == (1 if case[0] == "one-segment" else 0), (case[0], modes)
