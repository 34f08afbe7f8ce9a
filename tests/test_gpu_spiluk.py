"""ILU(k) on the GPU through the product library and the torch backend: the graphs of L and U and the level sets against the restated
reference loop, exact factors (bit for bit over NaN-seeded L_values / U_values), the knob sweep, the ILU identity bound on rounded
values, repeated numeric calls on one handle, a non-default stream, the 1e6 rule, and the factors as input of sptrsv_symbolic /
sptrsv_solve.  Inputs: tests/spiluk_cases.py at full size.

Worst ratios of identity_check measured on MI355X are recorded in profiles/spiluk/identity_ratios.txt."""
import numpy as np
import pytest

import kk_loader
import spiluk_cases as ic

pytestmark = pytest.mark.gpu

_ids = lambda p: repr(p) if isinstance(p, ic.Pattern) else "k%d" % p


@pytest.fixture(scope="module")
def gpu():
    kk = kk_loader.load()
    return kk, kk.torch_backend()


@pytest.mark.parametrize("fill_lev", [0, 1, 2])
@pytest.mark.parametrize("pat", ic.all_patterns(False), ids=repr)
def test_symbolic_matches_reference_loop(gpu, pat, fill_lev):
    kk, be = gpu
    for offset_dtype in (np.int32, np.int64):
        f = ic.Factored(kk, be, pat, fill_lev, offset_dtype, slack=(0, 5)[fill_lev % 2])
        ic.check_symbolic(f)
        f.close()


@pytest.mark.parametrize("pat,fill_lev", ic.exact_cases(False), ids=_ids)
def test_exact_factors(gpu, pat, fill_lev):
    kk, be = gpu
    for offset_dtype in (np.int32, np.int64):
        f = ic.Factored(kk, be, pat, fill_lev, offset_dtype)
        for dtype in (np.float64, np.float32):
            ic.check_exact(f, dtype)
        f.close()


# the long-row case of the sweep is c at emulator size (80 rows of up to 81 entries: beyond one pass of 64 lanes, and beyond the LDS cap
# of every lane count up to 16): one lane walking the 245-entry rows of the full c takes half a second per call.  The full c meets
# every lane count in test_long_rows_under_every_lane_count.
@pytest.mark.parametrize("pat,fill_lev,offset_dtype", [(ic.cases(True)["c"][1], 0, np.int32), (ic.cases(False)["d"][0], 0, np.int64),
                                                       (ic.cases(False)["d"][1], 2, np.int32)],
                         ids=lambda p: repr(p) if isinstance(p, ic.Pattern) else (np.dtype(p).name if isinstance(p, type) else "k%d" % p))
def test_exact_factors_and_launch_counts_over_every_knob(gpu, pat, fill_lev, offset_dtype):
    kk, be = gpu
    ic.check_knob_sweep(kk, be, pat, fill_lev, (np.float64, np.float32), offset_dtype)


def test_long_rows_under_every_lane_count(gpu):
    kk, be = gpu
    f = ic.Factored(kk, be, ic.cases(False)["c"][1], 0, np.int64)
    for i, lanes in enumerate(ic.LANES):
        f.ih.set("lanes_per_row", lanes)
        ic.check_exact(f, (np.float64, np.float32)[i % 2])
        if lanes >= 16:
            ic.check_exact(f, (np.float32, np.float64)[i % 2])
    f.close()


def test_case_shapes(gpu):
    """the cases reach the paths they are meant for"""
    kk, be = gpu
    c = ic.cases(False)
    b = ic.Factored(kk, be, c["b"][0], 0)
    assert b.ih.get("max_level_rows") > 256 and 0 < b.ih.get("chained_levels") < b.ih.get_num_levels()          # wide levels and a chained tail
    d = ic.Factored(kk, be, c["d"][0], 0)
    assert d.ih.get_num_levels() == 3000 and d.ih.get("chained_levels") == 3000 and d.ih.get("launches") == 3   # more than chain_levels levels
    # c: rows beyond one pass of 64 lanes; beyond the LDS cap of every lane count up to 32 at k = 0, and of 64 lanes too at k = 1
    for k, lanes in ((0, 32), (1, 64)):
        f = ic.Factored(kk, be, c["c"][0], k)
        longest = int((np.diff(f.sym.L_row_map) + np.diff(f.sym.U_row_map)).max())
        assert longest > 64 and longest > f.ih.get("stage_entries_per_lane") * lanes
        assert f.ih.get("lanes_in_use") == 64
        f.close()
    # plan_bytes: one level as wide as the matrix costs 4 bytes per row (the reference's dense work array: level_maxrows x nrows ordinals)
    a = ic.Factored(kk, be, c["a"][0], 0)
    assert a.ih.get("max_level_rows") == 1000 and a.ih.get("plan_bytes") == 4 * 1000 + 16
    for name in ("a", "e27", "e7"):
        for k in (0, 2):
            f = ic.Factored(kk, be, c[name][0], k)
            assert 0 < f.ih.get("plan_bytes") <= 64 * (f.sym.n + f.sym.nnzL + f.sym.nnzU) + 4096
            f.close()
    e = ic.Factored(kk, be, c["e27"][0], 0)
    assert e.ih.get_num_levels() == 78 and e.ih.get("lanes_in_use") == 16                # the level sets of the 27-point lower triangle
    for f in (a, b, d, e):
        f.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("fill_lev", [0, 1, 2])
@pytest.mark.parametrize("pat", ic.all_patterns(False, ("b", "c", "e27", "e7")), ids=repr)
def test_rounded_values_meet_the_identity_bound(gpu, pat, fill_lev, dtype):
    kk, be = gpu
    A = pat.rounded.astype(dtype)
    f = ic.Factored(kk, be, pat, fill_lev)
    ic.identity_check(pat, f.sym, A, *f.numeric(A, dtype), dtype)
    f.close()


def test_two_numeric_calls_with_new_values_on_one_handle(gpu):
    kk, be = gpu
    pat = ic.cases(False)["e27"][1]
    f = ic.Factored(kk, be, pat, 0)
    A, L, U = pat.exact(0)
    lv, uv = f.numeric(A, np.float64)
    assert np.array_equal(lv, L) and np.array_equal(uv, U)
    lv, uv = f.numeric(-A, np.float64)                       # no second symbolic call: the handle keeps no values
    assert np.array_equal(lv, L) and np.array_equal(uv, -U)
    f.close()


def test_numeric_on_a_non_default_stream(gpu):
    import torch
    kk, be = gpu
    pat = ic.cases(False)["b"][1]
    f = ic.Factored(kk, be, pat, 1)
    A, L, U = pat.exact(1)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        assert be.stream() == stream.cuda_stream
        lv, uv = f.numeric(A, np.float64)
    assert np.array_equal(lv, L) and np.array_equal(uv, U)
    f.close()


@pytest.mark.parametrize("name,pat,values,fill_lev", ic.g_cases(), ids=[g[0] for g in ic.g_cases()])
def test_zero_pivots_become_1e6(gpu, name, pat, values, fill_lev):
    kk, be = gpu
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


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("pat,fill_lev", [(ic.cases(False)["b"][1], 2), (ic.cases(False)["e7"][0], 0)], ids=_ids)
def test_factors_are_valid_input_of_sptrsv(gpu, pat, fill_lev, dtype):
    """b = (L U) x* with the product formed in int64 (on 2 U, halved); spiluk, then sptrsv on L and on U, gives x* back bit for bit: the
    diagonal is stored, last in L and first in U"""
    kk, be = gpu
    A, L, U = pat.exact(fill_lev)
    sym = pat.symbolic(fill_lev)
    rng = np.random.default_rng(11)
    xstar = rng.integers(-2, 3, pat.n).astype(np.int64)
    Li, U2 = np.rint(L).astype(np.int64), np.rint(2 * U).astype(np.int64)
    assert np.array_equal(Li, L) and np.array_equal(U2, 2 * U)
    y2 = np.zeros(pat.n, dtype=np.int64)                    # 2 U x*
    np.add.at(y2, sym.U_rows, U2 * xstar[sym.U_entries])
    b2 = np.zeros(pat.n, dtype=np.int64)                    # 2 L U x*
    np.add.at(b2, sym.L_rows, Li * y2[sym.L_entries])
    bound = np.zeros(pat.n, dtype=np.int64)
    np.add.at(bound, sym.L_rows, np.abs(Li) * np.abs(y2[sym.L_entries]))
    ubound = np.zeros(pat.n, dtype=np.int64)
    np.add.at(ubound, sym.U_rows, np.abs(U2) * np.abs(xstar[sym.U_entries]))
    assert max(bound.max(), ubound.max()) < 2 ** 24          # every partial sum of both solves is exact in fp32
    f = ic.Factored(kk, be, pat, fill_lev)
    a = be.from_numpy(A.astype(dtype))
    lv = be.from_numpy(np.full(sym.nnzL, np.nan, dtype=dtype)); uv = be.from_numpy(np.full(sym.nnzU, np.nan, dtype=dtype))
    kk.spiluk_numeric(f.kh, fill_lev, f.A_row_map, f.A_entries, a, f.L_row_map, f.L_entries, lv, f.U_row_map, f.U_entries, uv)
    x = be.from_numpy((b2 / 2.0).astype(dtype))
    for lower, rm, ent, val in ((True, f.L_row_map, f.L_entries, lv), (False, f.U_row_map, f.U_entries, uv)):
        kh = kk.KokkosKernelsHandle(be)
        kh.create_sptrsv_handle("SEQLVLSCHD_TP1CHAIN", pat.n, lower)
        kk.sptrsv_symbolic(kh, rm, ent)
        kk.sptrsv_solve(kh, rm, ent, val, x, x)
        kh.destroy_sptrsv_handle()
    assert np.array_equal(be.to_numpy(x), xstar.astype(dtype))
    f.close()
