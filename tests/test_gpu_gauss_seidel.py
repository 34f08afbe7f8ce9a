"""Multicolor Gauss-Seidel on the GPU through the product library and the torch backend: the colouring against the restated greedy
colouring, supplied colours, exact sweeps (x1 bit for bit) for every algorithm and over the knob grid, composition and rank-2
identities bit for bit, the local rounding bound, ghost columns, the reference's convergence criterion, error statuses and an apply on
a non-default stream.  Inputs: tests/gauss_seidel_cases.py at full size."""
import numpy as np
import pytest

import kk_loader
import gauss_seidel_cases as gc
import sptrsv_cases as tc

pytestmark = pytest.mark.gpu

CASES = gc.all_cases(False)
DTYPES = (np.float64, np.float32)


@pytest.fixture(scope="module")
def gpu():
    kk = kk_loader.load()
    return kk, kk.torch_backend()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_colours_and_exact_sweeps(gpu, case):
    kk, be = gpu
    for k, offset_dtype in enumerate((np.int32, np.int64)):
        for threshold in ((0, 64) if case.name == "e" else (0,)):
            sm = gc.Smoother(kk, be, case, "GS_DEFAULT", offset_dtype, threshold)
            gc.check_coloring(sm)
            sm.symbolic()                                   # a second symbolic call gives the same arrays
            gc.check_coloring(sm)
            gc.check_exact(sm, DTYPES[k], "forward", 1.0, numeric=False)      # apply runs the numeric phase of a fresh analysis itself
            for dtype in DTYPES:
                for direction in gc.DIRECTIONS:
                    for omega in gc.OMEGAS:
                        gc.check_exact(sm, dtype, direction, omega)
                    gc.check_exact(sm, dtype, direction, 1.0, zero_x=True)
            sm.close()
        for algo in gc.ALGORITHMS[1:]:
            sm = gc.Smoother(kk, be, case, algo, offset_dtype)
            for direction in gc.DIRECTIONS:
                gc.check_exact(sm, DTYPES[k], direction, gc.OMEGAS[1 + k])
            sm.close()


def test_case_shapes(gpu):
    """the cases reach the paths they are meant for"""
    kk, be = gpu
    c = gc.cases(False)
    assert int(c["a"][0].colors.max()) == 1
    assert c["e"][0].row_len.max() > 300                    # beyond one pass of 64 lanes
    sm = gc.Smoother(kk, be, c["e"][0], threshold=64)
    assert sm.gh.get("long_rows") == 5
    assert 0 < sm.gh.get("chained_levels") < sm.gh.get_num_colors()                    # wide colours and a chained tail
    sm.gh.set("chain_rows", 0)
    assert sm.gh.get("tail_launches") >= 1                  # outside a chain the long rows launch on their own
    sm.close()
    sm = gc.Smoother(kk, be, c["c"][0])
    assert sm.gh.get_num_colors() >= 8 and sm.gh.get("max_level_rows") > 64 and sm.gh.get("chain_launches") >= 1
    sm.close()
    sm = gc.Smoother(kk, be, c["c-par"][0])
    assert sm.gh.get_num_colors() == 8 and sm.gh.get("launches") == 8
    sm.close()
    sm = gc.Smoother(kk, be, c["d"][0])
    assert sm.gh.get("max_level_rows") > 1024                                         # several workgroups per colour
    sm.close()
    sm = gc.Smoother(kk, be, c["i"][0])
    assert (sm.gh.get("launches"), sm.gh.get("chain_launches"), sm.gh.get("chained_levels")) == (1, 1, 70)
    sm.close()


def test_supplied_colours_are_validated(gpu):
    gc.check_supplied_colours(*gpu, False)


@pytest.mark.parametrize("case,offset_dtype", [(gc.cases(False)["e"][1], np.int32), (gc.cases(False)["i"][0], np.int64)],
                         ids=lambda p: repr(p) if isinstance(p, gc.Case) else np.dtype(p).name)
def test_exact_sweeps_and_launch_counts_over_every_knob(gpu, case, offset_dtype):
    kk, be = gpu
    gc.check_knob_sweep(kk, be, case, DTYPES, offset_dtype, tc.LANES, tc.CHAIN_ROWS, tc.CHAIN_LEVELS)


@pytest.mark.parametrize("case", gc.all_cases(False, ("c", "e", "g", "i")), ids=repr)
def test_composition_bit_for_bit(gpu, case):
    gc.check_composition(*gpu, case)


@pytest.mark.parametrize("case", gc.all_cases(False, ("c", "d", "e", "f", "g")), ids=repr)
def test_one_rounded_sweep_meets_the_local_bound(gpu, case):
    kk, be = gpu
    values, x0, y = case.rounded
    sm = gc.Smoother(kk, be, case)
    for dtype in DTYPES:
        for direction in gc.DIRECTIONS:
            x = sm.apply(direction, values, x0, y, dtype, omega=0.9)
            gc.local_bound_check(case, values.astype(dtype), x0.astype(dtype), y.astype(dtype), x, direction, dtype(0.9), dtype)
    sm.close()


@pytest.mark.parametrize("nv", [5, 17])
@pytest.mark.parametrize("layout", ["left", "right", "strided-left", "strided-right"])
def test_rank_2_columns_equal_rank_1(gpu, nv, layout):
    gc.check_rank2(*gpu, gc.cases(False)["g"][1], nv, layout, np.float64 if nv == 5 else np.float32)


def test_ghost_entries_are_read_and_come_back_unchanged(gpu):
    gc.check_ghost_entries(*gpu, False)


def test_symmetric_iterations_reduce_the_error(gpu):
    gc.check_convergence(*gpu, gc.cases(False)["c"][1])


def test_error_statuses(gpu):
    gc.check_statuses(*gpu, gc.cases(False)["d"][0])


def test_empty_matrix(gpu):
    gc.check_empty(*gpu, False)


def test_apply_on_a_non_default_stream(gpu):
    import torch
    kk, be = gpu
    case = gc.cases(False)["d"][1]
    sm = gc.Smoother(kk, be, case)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        assert be.stream() == stream.cuda_stream
        gc.check_exact(sm, np.float64, "forward", 1.5)
        gc.check_exact(sm, np.float32, "backward", 0.5)
    sm.close()
