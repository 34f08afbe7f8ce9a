"""Restarted GMRES on the GPU through the product library and the torch backend: the orthogonalisation kernels bit for bit against numpy
in longdouble over the shape grid, fuse 0 against fuse 1, the solver against the restated reference loop (CGS2 and MGS, both fuse
settings, int32 and int64 offsets), the invariants (true residual, Arnoldi relation, loss of orthogonality), the three preconditioner
kinds with an LUPrec built from spiluk's output, errors and handle state.  Inputs: tests/gmres_cases.py at full size."""
import numpy as np
import pytest

import kk_loader
import gmres_cases as gc

pytestmark = pytest.mark.gpu

SMALL = False
NAMES = [c.name for c in gc.cases(SMALL)]
DT = dict(ids=lambda d: np.dtype(d).name)


@pytest.fixture(scope="module")
def gpu():
    kk = kk_loader.load()
    return kk, kk.torch_backend()


# 1 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", gc.DTYPES, **DT)
@pytest.mark.parametrize("n", gc.KERNEL_N)
def test_kernels_bit_for_bit(gpu, n, dtype):
    kk, be = gpu
    for k in gc.KERNEL_K:
        gc.check_kernels_exact(kk, be, n, k, dtype)


@pytest.mark.parametrize("dtype", gc.DTYPES, **DT)
def test_kernels_inf_nan(gpu, dtype):
    kk, be = gpu
    for fuse in (0, 1):
        gc.check_kernels_nonfinite(kk, be, dtype, fuse)


# 2 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", gc.DTYPES, **DT)
def test_fuse_0_equals_fuse_1(gpu, dtype):
    kk, be = gpu
    for n, k in ((65, 9), (1000, 17), (4097, 50), (4097, 64), (1000, 65), (100000, 33), (1, 1)):
        gc.check_fuse_equivalence(kk, be, n, k, dtype)


# 3 and 4 ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ortho", ["CGS2", "MGS"])
@pytest.mark.parametrize("dtype", gc.DTYPES, **DT)
@pytest.mark.parametrize("name", NAMES)
def test_solver_against_the_restated_loop(gpu, name, dtype, ortho):
    kk, be = gpu
    lu = gc.case(SMALL, name).precond == "lu"
    r1, ratio = gc.check_solver(kk, be, SMALL, name, dtype, ortho, fuse=1, lu_from_spiluk=lu)
    if ratio is not None:
        print("loss of orthogonality over the restated loop's: %s %s %.3g" % (name, np.dtype(dtype).name, ratio))
    if ortho == "MGS":                                                         # the knob "fuse" has no part in MGS
        return
    r0, _ = gc.check_solver(kk, be, SMALL, name, dtype, ortho, fuse=0, offset_dtype=np.int64, rows_per_group=64)
    if r1.cycles > 0:
        assert (r1.last_fused, r0.last_fused) == (1, 0)


def test_fuse_changes_no_bit_of_a_solve(gpu):
    kk, be = gpu
    for name in ("conv2d-m10", "tri"):
        c = gc.case(SMALL, name)
        for dtype in gc.DTYPES:
            tol = gc.reference(SMALL, name, dtype, "CGS2")[0]
            a, b, b2 = (gc.solve(kk, be, c, dtype, "CGS2", tol, fuse=f) for f in (0, 1, 1))
            for x in (b, b2):
                assert a.X.tobytes() == x.X.tobytes() and a.H.tobytes() == x.H.tobytes() and a.V.tobytes() == x.V.tobytes()
            assert a.launches > b.launches and a.host_syncs == b.host_syncs


# 5 ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("from_spiluk", [False, True])
@pytest.mark.parametrize("dtype", gc.DTYPES, **DT)
def test_preconditioners(gpu, dtype, from_spiluk):
    kk, be = gpu
    gc.check_preconditioners(kk, be, SMALL, dtype, lu_from_spiluk=from_spiluk)


# 6 ----------------------------------------------------------------------------------------------------------------------------------

def test_errors_and_state(gpu):
    kk, be = gpu
    gc.check_errors_and_state(kk, be, SMALL)


def test_solve_on_a_side_stream(gpu):
    """the solve runs on the backend's current stream and leaves the same bits there"""
    import torch
    kk, be = gpu
    c = gc.case(SMALL, "conv2d-lu")
    tol = gc.reference(SMALL, c.name, np.float64, "CGS2")[0]
    a = gc.solve(kk, be, c, np.float64, "CGS2", tol)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = gc.solve(kk, be, c, np.float64, "CGS2", tol)
    s.synchronize()
    assert a.X.tobytes() == b.X.tobytes() and a.num_iters == b.num_iters
