"""KokkosSparse::Experimental::spgemm_jacobi on the GPU through the product library and the torch backend: the checks of
tests/test_emu_spgemm_jacobi.py (tests/spgemm_jacobi_cases.py) -- structure and values `==` the definition on exactly representable inputs for
both offset and both value types, bit for bit the documented composition and the rounding bound on rounded ones, rows of B of every
special length under every lane width (query 24), rows of C around every power of two, both forms of the epilogue (query 25), special
values, statuses, the row-partitioned form with both ranks in this process, and the smoothed prolongator of the 7-point 12^3 lattice."""
import numpy as np
import pytest

import kk_loader
import spgemm_jacobi_cases as jc

pytestmark = pytest.mark.gpu

OPERANDS = ("lat27_squared", "lat7_prolongator", "rmat_squared", "unsorted_B", "diagonal_A")


@pytest.fixture(scope="module")
def gpu():
    kk = kk_loader.load()
    return kk, kk.torch_backend()


@pytest.fixture(scope="module")
def operands(gpu):
    return jc.exact_operands(*gpu)


@pytest.mark.parametrize("name", OPERANDS)
@pytest.mark.parametrize("odt,vdt", jc.TYPE_GRID, ids=lambda t: np.dtype(t).name)
def test_exactly_the_definition(gpu, operands, name, odt, vdt):
    kk, be = gpu
    jc.check_exact(kk, be, name, *operands[name], odt, vdt, expect_fast=name not in ("unsorted_B", "lat27_squared"))


@pytest.mark.parametrize("name", OPERANDS)
@pytest.mark.parametrize("odt,vdt", jc.TYPE_GRID, ids=lambda t: np.dtype(t).name)
def test_the_documented_composition_bit_for_bit_and_the_rounding_bound(gpu, operands, capfd, name, odt, vdt):
    """bits are compared wherever one wave owns a row's accumulator -- every operand but R-MAT squared, whose long rows take the value kernels
    that several waves add into with floating-point atomics: there two numeric calls differ from each other (spgemm_jacobi_cases.check_rounded)
    and the bound alone holds"""
    kk, be = gpu
    share, bits = jc.check_rounded(kk, be, name, *operands[name], odt, vdt, capfd=capfd)
    assert share <= 1.0 and bits == (name != "rmat_squared")


@pytest.mark.parametrize("lanes", jc.WIDTHS)
@pytest.mark.parametrize("odt,vdt", jc.TYPE_GRID[:2], ids=lambda t: np.dtype(t).name)
def test_rows_of_b_under_every_lane_width(gpu, lanes, odt, vdt):
    kk, be = gpu
    jc.check_widths(kk, be, lanes, odt, vdt)


@pytest.mark.parametrize("odt,vdt", jc.TYPE_GRID, ids=lambda t: np.dtype(t).name)
def test_bisection_of_rows_of_c_of_every_length(gpu, odt, vdt):
    kk, be = gpu
    jc.check_bisection(kk, be, odt, vdt)


def test_the_form_of_the_epilogue(gpu):
    jc.check_forms(*gpu)


def test_empty_operands(gpu):
    jc.check_empty(*gpu)


@pytest.mark.parametrize("odt,vdt", jc.TYPE_GRID, ids=lambda t: np.dtype(t).name)
def test_special_values(gpu, odt, vdt):
    kk, be = gpu
    jc.check_special(kk, be, odt, vdt)


def test_statuses(gpu):
    jc.check_statuses(*gpu)


@pytest.mark.parametrize("odt,vdt", jc.TYPE_GRID[:2], ids=lambda t: np.dtype(t).name)
def test_row_partitioned(gpu, odt, vdt):
    kk, be = gpu
    jc.check_dist(kk, be, odt, vdt)


@pytest.mark.parametrize("vdt", [np.float64, np.float32], ids=lambda t: np.dtype(t).name)
def test_smoothed_prolongator(gpu, vdt):
    kk, be = gpu
    jc.check_use(kk, be, vdt)
