"""The plain numpy reference of y = beta y0 + alpha op(A) x that the exact-value SpMV checks compare with (parity_cases.spmv_by_products) is itself
pinned: against the oracle's serial SpMV on signed values (within the bound of any summation order), against scipy where scipy is installed, on a
case worked out by hand (duplicates, an empty row, a stored zero times Inf, Inf - Inf, alpha = 0), and the rule that picks the number of value
bits (spmv_value_bits) against random orders of summation in the vector type."""
import numpy as np
import pytest

import oracle
import parity_cases as pc


def _cases():
    yield "27-pt", oracle.laplace3d("FE", 6, 5, 4)
    yield "random, unsorted with duplicates", oracle.random_crs(300, 170, 9, variance=6, seed=5)
    yield "wide", oracle.random_crs(40, 900, 30, variance=25, seed=6)
    yield "hubs", pc.hub_matrix(200, 1500, 4, {5: 700, 17: 129}, seed=3)
    yield "empty rows", pc.mv6_cases()[4][1]
    yield "no entries", oracle.random_crs(9, 7, 0, seed=1)


@pytest.mark.parametrize("mode", ["N", "C", "T", "H"])
def test_against_the_oracle(mode):
    rng = np.random.default_rng(11)
    u = 2.0 ** -53
    for name, A0 in _cases():
        v = rng.uniform(-50, 50, A0.nnz)
        A = oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, v)
        nin, nout = (A0.nrows, A0.ncols) if mode in "TH" else (A0.ncols, A0.nrows)
        for alpha, beta in ((1.0, 0.0), (-2.0, 0.5), (3.0, -1.0), (0.0, 2.0)):
            x = rng.uniform(-1, 1, nin); y0 = rng.uniform(-1, 1, nout)
            Y, n, S = pc.spmv_by_products(A0, v, x, mode, alpha, beta, y0)
            gold = oracle.spmv_serial(mode, A, alpha, x, beta, y0.copy())
            m = (n + 2).astype(np.longdouble)
            assert (np.abs(gold.astype(np.longdouble) - Y) <= m * u / (1 - m * u) * (abs(alpha) * S + np.abs(beta * y0))).all(), (name, alpha, beta)
            assert n.sum() == A0.nnz and (n == (np.bincount(A0.entries, minlength=A0.ncols) if mode in "TH" else np.diff(A0.row_map))).all()
            X = rng.uniform(-1, 1, (nin, 3)); Y0 = rng.uniform(-1, 1, (nout, 3))
            Y2, n2, S2 = pc.spmv_by_products(A0, v, X, mode, alpha, beta, Y0)
            gold = oracle.spmv_mv_serial(mode, A, alpha, X, beta, Y0.copy())
            assert Y2.shape == (nout, 3) and (np.abs(gold.astype(np.longdouble) - Y2) <= m[:, None] * u / (1 - m[:, None] * u) * (abs(alpha) * S2 + np.abs(beta * Y0))).all(), (name, alpha, beta)
            for j in range(3):                              # a multivector is its columns
                Yj, _, Sj = pc.spmv_by_products(A0, v, X[:, j], mode, alpha, beta, Y0[:, j])
                assert np.array_equal(Yj, Y2[:, j]) and np.array_equal(Sj, S2[:, j])


def test_against_scipy():
    pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(12)
    for name, A0 in _cases():
        v = rng.uniform(-50, 50, A0.nnz)
        M = oracle.Crs(A0.nrows, A0.ncols, A0.row_map, A0.entries, v).to_scipy()
        for mode in "NT":
            nin, nout = (A0.nrows, A0.ncols) if mode == "T" else (A0.ncols, A0.nrows)
            x = rng.uniform(-1, 1, nin); y0 = rng.uniform(-1, 1, nout)
            Y, n, S = pc.spmv_by_products(A0, v, x, mode, -2.0, 0.5, y0)
            ref = 0.5 * y0 - 2.0 * ((M.T if mode == "T" else M) @ x)
            assert np.allclose(Y.astype(np.float64), ref, rtol=1e-11, atol=1e-11), (name, mode)


def test_by_hand():
    # row 0 = {1: 2, 0: 3, 1: -2} (unsorted, column 1 twice), row 1 empty, row 2 = {2: 0.0} (a stored zero), row 3 = {0: 1, 2: -1}
    A = oracle.Crs(4, 3, np.array([0, 3, 3, 4, 6]), np.array([1, 0, 1, 2, 0, 2], dtype=np.int32), np.zeros(6))
    v = np.array([2.0, 3.0, -2.0, 0.0, 1.0, -1.0])
    y0 = np.array([1.0, 2.0, 3.0, 4.0])
    x = np.array([1.0, 5.0, -2.0])
    Y, n, S = pc.spmv_by_products(A, v, x, "N", 2.0, 0.5, y0)
    assert n.tolist() == [3, 0, 1, 2] and S.tolist() == [23.0, 0.0, 0.0, 3.0]
    assert Y.tolist() == [6.5, 1.0, 1.5, 8.0]                 # 2 (10 + 3 - 10) + 0.5, 0 + 1, 2 (0 * -2) + 1.5, 2 (1 + 2) + 2
    Y, n, S = pc.spmv_by_products(A, v, x, "C", 2.0, 0.0, np.full(4, np.nan))
    assert Y.tolist() == [6.0, 0.0, 0.0, 6.0]                 # beta = 0: y0 is not read
    # Inf in x: 3 * Inf beside products that cancel; a stored zero times Inf; Inf - Inf
    xi = np.array([np.inf, 5.0, np.inf])
    Y, n, S = pc.spmv_by_products(A, v, xi, "N", 2.0, 0.5, y0)
    assert Y[0] == np.inf and Y[1] == 1.0 and np.isnan(Y[2]) and np.isnan(Y[3])
    Y, _, _ = pc.spmv_by_products(A, v, -xi, "N", 2.0, 0.5, y0)
    assert Y[0] == -np.inf
    # alpha = 0: beta y0 whatever A and x hold; beta = 0 as well: zero
    vi = np.array([np.nan, np.inf, -2.0, 0.0, -np.inf, -1.0])
    assert pc.spmv_by_products(A, vi, xi, "N", 0.0, -1.0, y0)[0].tolist() == [-1.0, -2.0, -3.0, -4.0]
    assert pc.spmv_by_products(A, vi, np.array([np.inf, 1.0, np.nan, -np.inf]), "T", 0.0, 0.0, np.full(3, np.nan))[0].tolist() == [0.0, 0.0, 0.0]
    # transposed: column 0 = 3 x0 + 1 x3, column 1 = 2 x0 - 2 x0, column 2 = 0.0 x2 - 1 x3
    xt = np.array([1.0, 2.0, 3.0, 4.0])
    Y, n, S = pc.spmv_by_products(A, v, xt, "T", 1.0, 0.0, np.zeros(3))
    assert Y.tolist() == [7.0, 0.0, -4.0] and n.tolist() == [2, 2, 2] and S.tolist() == [7.0, 4.0, 4.0]
    Y, _, _ = pc.spmv_by_products(A, v, np.array([1.0, np.inf, np.inf, 4.0]), "H", 1.0, 0.0, np.zeros(3))
    assert Y[0] == 7.0 and Y[1] == 0.0 and np.isnan(Y[2])       # the x of the empty row reaches nothing; 0.0 * Inf is NaN
    # rank 2
    Y, n, S = pc.spmv_by_products(A, v, np.stack([x, xi], axis=1), "N", 2.0, 0.5, np.stack([y0, y0], axis=1))
    assert Y[:, 0].tolist() == [6.5, 1.0, 1.5, 8.0] and Y[0, 1] == np.inf and np.isnan(Y[2:, 1]).all()


def test_value_bits_rule():
    assert pc.spmv_value_bits(27, np.float64) == 20 and pc.spmv_value_bits(27, np.float32) == 7 and pc.spmv_value_bits(27, np.float64, np.float32) == 10
    assert pc.spmv_value_bits(3000, np.float32) == 4 and pc.spmv_value_bits(7000, np.float32) == 3 and pc.spmv_value_bits(1 << 16, np.float64) == 16
    assert pc.spmv_n_max(pc.hub_matrix(50, 400, 3, {7: 130}, seed=1), "N") == 130 and pc.spmv_n_max(oracle.laplace1d(10), "T") == 3


@pytest.mark.parametrize("vec_dtype,n", [(np.float32, 3000), (np.float64, 40000)], ids=["fp32", "fp64"])
def test_value_bits_make_every_order_exact(vec_dtype, n):
    """one long row: y = beta y0 + sum of v (alpha x), the scaling inside every term as the transposed kernels do it, accumulated one by
    one in the vector type in random orders.  With b bits (spmv_value_bits) every order gives the bits of the long-double sum; with b + 3
    bits -- values in the upper half of their range, one sign, the worst case the rule is made for -- the orders disagree."""
    dt = np.dtype(vec_dtype)
    b = pc.spmv_value_bits(n, dt)
    assert b >= 2
    rng = np.random.default_rng(5)
    for bits, same in ((b, True), (b + 3, False)):
        v = rng.integers(1 << (bits - 1), 1 << bits, size=n).astype(np.float64) * 2.0 ** -4
        x = rng.integers(1 << (bits - 1), 1 << bits, size=n).astype(np.float64) * 2.0 ** -3
        y0 = float(rng.integers(1 << (bits - 1), 1 << bits)) * 2.0 ** -2
        alpha, beta = 3.0, -2.0
        assert np.array_equal(v.astype(dt), v) and np.array_equal(x.astype(dt), x)
        exact = np.longdouble(beta) * y0 + (v.astype(np.longdouble) * (np.longdouble(alpha) * x.astype(np.longdouble))).sum()
        outs = set()
        for rep in range(12):
            p = rng.permutation(n)
            terms = np.concatenate([[dt.type(beta) * dt.type(y0)], v.astype(dt)[p] * (dt.type(alpha) * x.astype(dt)[p])]).astype(dt)
            outs.add(float(np.add.accumulate(terms, dtype=dt)[-1]))
        if same:
            assert outs == {float(exact)} and np.longdouble(float(exact)) == exact, (bits, outs, exact)
        else:
            assert len(outs) > 1, (bits, outs)
