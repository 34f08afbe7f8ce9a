"""The plain numpy reference of C = A * B that the exact-value SpGEMM checks compare with (parity_cases.spgemm_by_products) is itself pinned:
against the oracle's SPGEMM_DEBUG on small cases of the suite (structure identical, values within the bound of any fp64 summation order), against
scipy where scipy is installed, and on a product worked out by hand (duplicates, a cancelling sum, unsorted rows)."""
import numpy as np
import pytest

import oracle
import parity_cases as pc


def _cases():
    L = oracle.laplace3d("FE", 6, 5, 4)
    yield "27-pt squared", L, L
    yield "random, sorted", pc.randomized(oracle.random_crs(400, 320, 16, variance=10, seed=3, sorted_rows=True)), pc.randomized(oracle.random_crs(320, 240, 20, variance=12, seed=4, sorted_rows=True))
    yield "unsorted with duplicates", pc.randomized(oracle.random_crs(100, 50, 8, seed=5)), pc.randomized(oracle.random_crs(50, 160, 30, seed=6))
    yield "all bins", *pc.all_bins_operands()
    _, _, R, AP = pc.galerkin_operands(8)
    yield "Galerkin R (A P)", R, AP
    yield "empty A", pc.randomized(oracle.random_crs(10, 10, 0, seed=1, sorted_rows=True)), pc.randomized(oracle.random_crs(10, 10, 2, seed=2, sorted_rows=True))


@pytest.mark.parametrize("signed", [False, True])
def test_against_the_oracle(signed):
    rng = np.random.default_rng(7)
    for name, A, B in _cases():
        if signed:
            A = oracle.Crs(A.nrows, A.ncols, A.row_map, A.entries, rng.uniform(-50, 50, A.nnz))
            B = oracle.Crs(B.nrows, B.ncols, B.row_map, B.entries, rng.uniform(-50, 50, B.nnz))
        rm, ent, sums, n, S = pc.spgemm_by_products(A, B)
        gold = oracle.spgemm(A, B)
        assert np.array_equal(rm, gold.row_map) and np.array_equal(ent, gold.entries), name
        u = 2.0 ** -53
        m = (n + 1).astype(np.longdouble)
        assert (np.abs(gold.values.astype(np.longdouble) - sums) <= m * u / (1 - m * u) * S).all(), name
        assert (S >= np.abs(sums)).all() and (n >= 1).all()


def test_against_scipy():
    sp = pytest.importorskip("scipy.sparse")
    for name, A, B in _cases():
        A, B = pc.randomized(A, seed=1), pc.randomized(B, seed=2)          # values in [1, 50): scipy drops an entry whose sum is 0.0, the library keeps it
        rm, ent, sums, n, S = pc.spgemm_by_products(A, B)
        Cs = (A.to_scipy() @ B.to_scipy()).tocsr()
        Cs.sum_duplicates(); Cs.sort_indices()
        assert np.array_equal(rm, Cs.indptr) and np.array_equal(ent, Cs.indices), name
        assert np.allclose(sums.astype(np.float64), Cs.data, rtol=1e-12, atol=0), name


def test_by_hand():
    # A = [[2 (col 1), 3 (col 0), -2 (col 1)], [], [1 (col 2)]]: unsorted, column 1 twice.  B row 0 = {4: 5}, row 1 = {0: 7, 4: 1, 0: -7}, row 2 = {}
    A = oracle.Crs(3, 3, np.array([0, 3, 3, 4]), np.array([1, 0, 1], dtype=np.int32).tolist() + [2], np.array([2.0, 3.0, -2.0, 1.0]))
    B = oracle.Crs(3, 5, np.array([0, 1, 4, 4]), np.array([4, 0, 4, 0], dtype=np.int32), np.array([5.0, 7.0, 1.0, -7.0]))
    rm, ent, sums, n, S = pc.spgemm_by_products(A, B)
    assert rm.tolist() == [0, 2, 2, 2] and ent.tolist() == [0, 4]
    assert n.tolist() == [4, 3]                          # column 0: 2*7, 2*-7, -2*7, -2*-7; column 4: 2*1, 3*5, -2*1
    assert sums.tolist() == [0.0, 15.0] and S.tolist() == [56.0, 19.0]


def test_value_bits():
    assert pc.value_bits(1, np.float64) == 20 and pc.value_bits(83, np.float64) == 20 and pc.value_bits(83, np.float32) == 8
    assert pc.value_bits(1 << 14, np.float64) == 19 and pc.value_bits(2, np.float32) == 11
    rng = np.random.default_rng(0)
    v = pc.exact_values(rng, 1000, 8)
    assert (v != 0).all() and (np.abs(v) < 16).all() and (v * 16 == np.round(v * 16)).all() and (v < 0).any() and (v > 0).any()
