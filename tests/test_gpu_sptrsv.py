"""Sparse triangular solve on the GPU through the product library and the torch backend: level sets against the restated reference
loops, exact values (x* bit for bit over a NaN-seeded x, and with x aliased to b), the knob sweep, the backward-error bound on rounded
values, repeated solves on one handle and a solve on a non-default stream.  Inputs: tests/sptrsv_cases.py at full size."""
import numpy as np
import pytest

import kk_loader
import sptrsv_cases as sc

pytestmark = pytest.mark.gpu

TRIANGLES = sc.all_triangles(False)
ALGOS = ["SEQLVLSCHD_RP", "SEQLVLSCHD_TP1", "SEQLVLSCHD_TP1CHAIN"]


@pytest.fixture(scope="module")
def gpu():
    kk = kk_loader.load()
    return kk, kk.torch_backend()


@pytest.mark.parametrize("tri", TRIANGLES, ids=repr)
def test_level_sets_and_exact_values(gpu, tri):
    kk, be = gpu
    for k, offset_dtype in enumerate((np.int32, np.int64)):
        an = sc.Analysed(kk, be, tri, ALGOS[2], offset_dtype)
        sc.check_level_sets(an)
        for dtype in (np.float64, np.float32):
            sc.check_exact(an, dtype)
            sc.check_exact(an, dtype, alias=True)
        an.close()
        for algo in ALGOS[:2]:
            an = sc.Analysed(kk, be, tri, algo, offset_dtype)
            sc.check_exact(an, (np.float64, np.float32)[k])
            an.close()


def test_case_shapes(gpu):
    """the cases reach the paths they are meant for"""
    kk, be = gpu
    c = sc.cases(False)
    e = sc.Analysed(kk, be, c["e"][0])
    assert e.th.get_num_levels() == 78 and e.th.get("max_level_rows") == 36           # nx + 2 (ny - 1) + 4 (nz - 1) on 12 x 12 x 12
    d = sc.Analysed(kk, be, c["d"][0])
    assert d.th.get_num_levels() == 3000 and d.th.get("chained_levels") == 3000 and d.th.get("launches") == 3   # more than chain_levels levels
    b = sc.Analysed(kk, be, c["b"][0])
    assert b.th.get("max_level_rows") > 256 and 0 < b.th.get("chained_levels") < b.th.get_num_levels()          # wide levels and a chained tail
    assert int(np.diff(c["c"][0].row_map).max()) > 64                                  # rows beyond one pass of 64 lanes
    for an in (e, d, b):
        an.close()


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("tri,offset_dtype", [(sc.cases(False)["c"][1], np.int32), (sc.cases(False)["c"][2], np.int64),
                                              (sc.cases(False)["d"][1], np.int64), (sc.cases(False)["d"][2], np.int32)],
                         ids=lambda p: repr(p) if isinstance(p, sc.Triangle) else np.dtype(p).name)
def test_exact_values_and_launch_counts_over_every_knob(gpu, tri, offset_dtype, algo):
    kk, be = gpu
    sc.check_knob_sweep(kk, be, tri, (np.float64, np.float32), offset_dtype, algos=(algo,))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("tri", sc.all_triangles(False, "bce"), ids=repr)
def test_rounded_values_meet_the_backward_error_bound(gpu, tri, dtype):
    kk, be = gpu
    values, b = (a.astype(dtype) for a in tri.rounded)
    for algo in ALGOS:
        an = sc.Analysed(kk, be, tri, algo, np.int32)
        x = an.solve(values, b, dtype)
        sc.residual_check(tri, values, b, x, dtype)
        an.close()


def test_two_solves_with_new_values_on_one_handle(gpu):
    kk, be = gpu
    tri = sc.cases(False)["e"][3]
    an = sc.Analysed(kk, be, tri)
    values, b, xstar = tri.exact
    assert np.array_equal(an.solve(values, b, np.float64), xstar)
    assert np.array_equal(an.solve(-values, b, np.float64), -xstar)          # no second symbolic call: the handle keeps no values
    assert np.array_equal(an.solve(2.0 * values, b, np.float64), xstar / 2.0)
    an.close()


def test_solve_on_a_non_default_stream(gpu):
    import torch
    kk, be = gpu
    tri = sc.cases(False)["b"][1]
    an = sc.Analysed(kk, be, tri)
    values, b, xstar = tri.exact
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        assert be.stream() == stream.cuda_stream
        x = an.solve(values, b, np.float64)
    assert np.array_equal(x, xstar)
    an.close()
