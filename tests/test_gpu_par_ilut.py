"""ParILUT on the GPU through the product library and the torch backend: the steps bit for bit on exact inputs over both offset types, both
value types and every lane count, the radix select against numpy.partition, the whole loop against the restated reference loop within the
measured tolerance (recipe d up to n = 2000), run-to-run bit identity, par_ilut to LUPrec to gmres, error statuses.  Inputs:
tests/par_ilut_cases.py at full size."""
import numpy as np
import pytest

import kk_loader
import par_ilut_cases as pc

pytestmark = pytest.mark.gpu

CASES = pc.loop_cases(False)
LANES = (1, 2, 4, 8, 16, 32, 64)


@pytest.fixture(scope="module")
def gpu():
    kk = kk_loader.load()
    return kk, kk.torch_backend()


def test_reference_fixture(gpu):
    pc.check_fixture(*gpu)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("kind", ["band", "arrow"])
def test_steps_bit_for_bit(gpu, kind, lanes):
    kk, be = gpu
    for offset_dtype, dtype in ((np.int32, np.float64), (np.int64, np.float32), (np.int32, np.float32), (np.int64, np.float64)):
        pc.check_steps(kk, be, kind, offset_dtype, dtype, lanes)


@pytest.mark.parametrize("count", [1500, 5000])
def test_select_equals_numpy_partition(gpu, count):
    kk, be = gpu
    for dtype in (np.float64, np.float32):
        pc.check_select(kk, be, count, dtype)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_whole_loop_matches_reference_loop(gpu, case):
    kk, be = gpu
    pc.check_loop(kk, be, case, np.int32, np.float64)
    pc.check_loop(kk, be, case, np.int64, np.float32)


@pytest.mark.parametrize("lanes", [1, 16, 64])
def test_whole_loop_other_lane_counts(gpu, lanes):
    kk, be = gpu
    for case in (CASES[7], CASES[9]):                          # recipe d and the arrow: staged and unstaged L rows
        pc.check_loop(kk, be, case, np.int32, np.float64, lanes)
        pc.check_loop(kk, be, case, np.int32, np.float32, lanes)


def test_run_to_run_bit_identity(gpu):
    kk, be = gpu
    assert CASES[-1].name == "e-arrow300"
    f = pc.Factored(kk, be, CASES[-1])
    f.numeric(np.float64)
    assert f.ih.get("max_product_row") > 256                   # past the row length one wave of the SpGEMM accumulates alone
    f.close()
    for case in (CASES[8], CASES[9], CASES[-1]):               # n = 2000, the arrow, and the arrow whose L * U has a row of 300 entries
        for dtype in (np.float64, np.float32):
            runs = []
            for _ in range(3):
                f = pc.Factored(kk, be, case)
                runs.append(f.numeric(dtype))
                f.close()
            for L, U in runs[1:]:
                for a, b in ((L, runs[0][0]), (U, runs[0][1])):
                    assert a.row_map.tobytes() == b.row_map.tobytes() and a.entries.tobytes() == b.entries.tobytes()
                    assert np.asarray(a.values).tobytes() == np.asarray(b.values).tobytes()


def test_par_ilut_as_preconditioner_of_gmres(gpu):
    pc.check_precond(*gpu)


def test_error_statuses(gpu):
    pc.check_statuses(*gpu)


def test_repeated_numeric_with_new_values(gpu):
    kk, be = gpu
    pc.check_repeated_numeric(kk, be, np.float64)
    pc.check_repeated_numeric(kk, be, np.float32)


def test_numeric_on_a_side_stream(gpu):
    """the factorisation runs on the backend's current stream and leaves the same bits there"""
    import torch
    kk, be = gpu
    f = pc.Factored(kk, be, CASES[6])
    a = f.numeric(np.float64)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = f.numeric(np.float64)
    s.synchronize()
    for x, y in zip(a, b):
        assert x.entries.tobytes() == y.entries.tobytes() and np.asarray(x.values).tobytes() == np.asarray(y.values).tobytes()
    f.close()
