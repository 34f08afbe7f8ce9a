"""SpGEMM values on the GPU (`-m gpu`), exactly: every value kernel of the numeric phase against a plain numpy reference (long-double sums
of the expanded products, parity_cases.spgemm_by_products) on inputs whose every partial sum is representable, so that the comparison is
`==` -- signed values, sums that cancel to a stored zero, Inf / NaN / explicit zeros and numeric reuse after them -- and within the
textbook bound gamma_(n+1) sum|a * b| on signed real values.  Every case proves the kernel it reached from the library's verbose lines, and a
set of cases must have reached every bin and every value kernel (see parity_cases.check_spgemm_values)."""
import numpy as np
import pytest

import parity_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    import ctypes as C
    b = pc.kk.torch_backend()
    name = C.create_string_buffer(256); g = C.c_int(); cus = C.c_int()
    pc.kk._capi.check(b.lib, b.lib.kkamd_device_info(name, 256, C.byref(g), C.byref(cus)))
    assert g.value == 1, "libkkamd.so is built for gfx950 only; found %s" % name.value.decode()
    return b


@pytest.mark.parametrize("value_dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("mode", ["signed", "cancelling", "special", "bound"])
def test_spgemm_values_through_every_kernel(be, capfd, mode, value_dtype):
    pc.check_spgemm_values(be, capfd, mode, value_dtype)


def test_sort_and_merge_sums_exactly(be):
    pc.check_sort_and_merge_exact(be)
