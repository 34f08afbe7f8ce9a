"""SpMV values on the GPU (`-m gpu`), exactly: every route of rank 1, rank 2 and spmv_struct against a plain numpy reference (long-double sums of the
expanded products, parity_cases.spmv_by_products) on inputs whose every partial sum is representable, so that the comparison is `==` whatever the order
of summation -- signed values, rows that cancel to exactly zero from large terms, Inf / NaN / stored zeros in x and in A.values and finite values written
back under a live handle -- and within the per-entry bound gamma_(n+2) (|alpha| sum|a x| + |beta y0|) on signed real values.  Every case proves its route
by plan queries, with every type pair it accepts, and every route of a table must have been proved with the offset type of the test (see
parity_cases.check_spmv_values).

Largest error / bound per route in mode "bound" (only <= 1 is asserted), full tables, every type pair, both offset types, the kernels compiled for
the SIMT emulator (tests/emu):
  rank 1  vector kernel: no handle 0.30, FAST_SETUP 1 / 4 / 64 lanes 0.34 / 0.33 / 0.29; plain tiles 1024 / 2048 / 4096 ragged 0.42 / 0.57 / 0.54, 1024
          full 0.60; code tiles 0.11; staged-x 0.17; pattern tiles 27-pt from the matrix 0.16, through codes 0.18, 9-pt perturbed 0.35, 5-pt empty rows
          0.44; mixed 0.23; march 0.36, with gather rows 0.33; column slab atomic 0.30, deterministic 0.37; MERGE_PATH 0.31, NATIVE 0.30,
          NATIVE_MERGE_PATH 0.33; transposed: no handle 0.88, atomics 0.83, cached transpose 0.81
  rank 2  generic 0.41; gather nt 0 / 1 0.27 / 0.29; long rows 0.45; mv3 0.19; mv4 27-pt 0.22, 7-pt 0.41, 19-pt 0.30, 11-pt 0.30; mv5 32 x 32 blocks 0.11,
          5 x 5 blocks 0.47; mv6 0.74; transposed: no handle 0.49, atomics 0.42, cached transpose 0.47
  struct  1-D 0.50, 2-D FD 0.48, 2-D FE 0.30, 3-D FD 0.36, 3-D FE 0.17, 2-D FE with extra entries 0.25"""
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


@pytest.mark.parametrize("offset_dtype", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("kind", ["rank1", "rank2", "struct"])
@pytest.mark.parametrize("how", pc.VALUE_MODES)
def test_spmv_values_on_every_route(be, how, kind, offset_dtype):
    # every route of the table with every type pair it accepts, proved with this offset type
    pc.check_spmv_values(be, how, kind, offsets=(offset_dtype,))
