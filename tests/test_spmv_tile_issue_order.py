"""The planned rank-1 kernel's order of issue (kk_spmv.hip, spmv_stream3_kernel): every load of a tile that depends on the tile index alone is
requested unconditionally before any vector-memory wait -- the row bounds and the old y from a row clamped into the tile's range, unused x chunks from
a clamped column -- and tiles of two to four segments pick their x entries with the segments' constants in scalar registers, tiles of five to eight
from the record in LDS, in batches.  None of that changes a value: the cases below are the smallest 27-point matrices whose tiles have one segment
(and a ragged last tile), two to four segments at both tile sizes, and five to eight segments next to tiles that keep their codes.  Each runs the
reference's comparator, the exact-value checks (signed values; Inf / NaN at the positions clamped loads aim at) and a bit-for-bit comparison with
the same handle without pattern records.  One body, two backends: the SIMT emulator (no GPU) and the gfx950 library (`-m gpu`).

The tile counts are properties of the plan (they hold before and after the kernel's change); they prove that a case reaches the tiles it is here for."""
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
    ("one-segment", (400, 4, 3), 16, 21, 20, 1, 0),             # one-segment tiles; ragged last tile
    ("2-4-segments", (160, 6, 4), 16, 19, 18, 1, 0),            # at most one line end per tile
    ("2-4-segments-2048", (80, 9, 5), 8, 38, 37, 1, 0),         # the same at the 2048 tile
    ("5-8-segments", (80, 9, 5), 16, 19, 11, 0, 8),             # two line ends per tile, next to tiles that keep their codes
]

_MATRICES = {}


def _matrix(dims):
    if dims not in _MATRICES:
        _MATRICES[dims] = oracle.laplace3d("FE", *dims)
    return _MATRICES[dims]


def _knobs(npt, pattern_codes=2):
    return {"window_codes_min_knnz": 0, "nnz_per_thread": npt, "pattern_codes": pattern_codes}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_parity_and_tile_counts(be, case):
    _, dims, npt, tiles, pat, plain, code = case
    A0 = _matrix(dims)
    for odt, vdt in ((np.int32, None), (np.int64, np.float32)):
        h = pc.check_spmv(be, A0, "N", 1.5, 0.5, "SPMV_DEFAULT", knobs=_knobs(npt), max_val=32.0, offset_dtype=odt, value_dtype=vdt)
        got = tuple(h.query(k) for k in ("tiles", "pattern_tiles", "plain_tiles", "code_tiles"))
        assert got == (tiles, pat, plain, code), (case[0], got)
        pc.check_spmv(be, A0, "N", 1.0, 0.0, "SPMV_DEFAULT", nans=True, knobs=_knobs(npt), max_val=32.0, offset_dtype=odt, value_dtype=vdt)


@pytest.mark.parametrize("how", ["signed", "special"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_exact_values(be, case, how):
    name, dims, npt = case[:3]
    pc.check_spmv_exact(be, _matrix(dims), how, algo="SPMV_DEFAULT", knobs=_knobs(npt), proof=lambda q: q("pattern_tiles") > 0, name=name)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
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
