"""MIS-2, MIS-2 aggregation and explicit coarsening on the GPU through the product library and the torch backend: the checks of
tests/test_emu_mis2.py at the sizes that cross the boundaries of the compaction (tests/mis2_cases.py, small=False: more than one
workgroup, more than 2,048 workgroup counts in one scan, the 4,000-vertex random graph, the 27-point 40^3 lattice), and the pipeline
the feature exists for: on that lattice the off-diagonal structure of R (A P), through the library's SpGEMM with P built from the
labels, equals graph_explicit_coarsen(compress) entry for entry.

The compaction scans one count per workgroup, not one flag per vertex, so its boundaries are 2,048 workgroups (one recursion of
kk_scan.h, crossed by lat5big and by every case at 64 lanes per vertex) and 2,048^2 workgroups (a second recursion), crossed by a
path of 8,400,000 vertices at 64 lanes per vertex.  The restatement takes several seconds there, so that case is compared with the
library's own result at the default width, which the other tests tie to the restatement."""
import numpy as np
import pytest

import kk_loader
import mis2_cases as mc

pytestmark = pytest.mark.gpu

CASES = mc.all_cases(False)


@pytest.fixture(scope="module")
def gpu():
    kk = kk_loader.load()
    return kk, kk.torch_backend()


def test_case_shapes(gpu):
    mc.check_shapes(False)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_the_set_and_its_rounds_match_the_restated_loops(gpu, case):
    kk, be = gpu
    # lat5big: MIS2_QUALITY on equal degrees decides about one lattice line per round; the restatement would take minutes
    algos = ("MIS2_FAST",) if case.name == "lat5big" else mc.ALGOS
    mc.check_mis(kk, be, case, np.int64 if case.name in ("lat7", "ghosts", "lat5big") else np.int32, algos)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_labels_match_the_restated_aggregation(gpu, case):
    kk, be = gpu
    mc.check_aggregation(kk, be, case, np.int64 if case.name in ("lat27", "selfloops") else np.int32)


@pytest.mark.parametrize("case", mc.all_cases(False, ("rand", "ghosts", "selfloops", "hub", "lat27big")), ids=repr)
def test_no_output_depends_on_the_lanes_per_vertex(gpu, case):
    kk, be = gpu
    mc.check_lanes(kk, be, case)


def test_two_level_scan_at_64_lanes(gpu):
    """64 lanes per vertex: four vertices per workgroup, so the 64,000-vertex lattice scans 32,000 counts"""
    kk, be = gpu
    g = mc.all_cases(False, ("lat27big",))[0]
    try:
        mc.set_lanes(be, 64)
        mc.check_mis(kk, be, g, algos=("MIS2_FAST",))
        mc.check_aggregation(kk, be, g)
    finally:
        mc.set_lanes(be, 0)


def test_three_level_scan_on_a_long_path(gpu):
    """8,400,000 vertices at 64 lanes per vertex: 2 * ceil(n / 4) + 1 = 4,200,001 workgroup counts in the first round, more than
    2,048^2, so the scan of kk_scan.h recurses twice through its workspace.  The set, the labels and the counts equal those of the
    default width (one lane per vertex on a path: 65,626 counts, one recursion)."""
    kk, be = gpu
    n = 8400000
    assert 2 * -(-n // 4) + 1 > 2048 * 2048
    ent = np.stack([np.arange(-1, n - 1, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32)], axis=1).reshape(-1)[1:-1]
    rm = np.concatenate([[0], np.cumsum(np.where((np.arange(n) == 0) | (np.arange(n) == n - 1), 1, 2))]).astype(np.int32)
    assert rm[-1] == ent.size == 2 * n - 2
    d_rm, d_ent = be.from_numpy(rm), be.from_numpy(np.ascontiguousarray(ent))
    got = []
    try:
        for lanes in (0, 64):
            mc.set_lanes(be, lanes)
            st, sa = {}, {}
            mis = be.to_numpy(kk.graph_d2_mis(d_rm, d_ent, "MIS2_FAST", backend=be, stats=st))
            lab, num = kk.graph_mis2_aggregate(d_rm, d_ent, backend=be, stats=sa)
            got.append((mis, be.to_numpy(lab), num, st["rounds"], sa["rounds"], sa["masked_rounds"], sa["secondary_aggregates"]))
    finally:
        mc.set_lanes(be, 0)
    a, b = got
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    assert a[0].size > n // 5 and (np.diff(a[0]) >= 3).all() and (np.diff(a[0]) <= 5).all()    # distance 2: independent and maximal on a path
    assert a[1].min() >= 0 and a[1].max() == a[2] - 1


@pytest.mark.parametrize("case", mc.all_cases(False, ("lat7", "rand", "ghosts", "selfloops", "ring", "hub", "lat27big")), ids=repr)
def test_explicit_coarsening_and_the_inverse_map(gpu, case):
    kk, be = gpu
    mc.check_coarsening(kk, be, case, np.int64 if case.name in ("rand", "ghosts") else np.int32)


def test_error_statuses(gpu):
    kk, be = gpu
    mc.check_statuses(kk, be, mc.all_cases(False, ("lat7",))[0])


def test_empty_graph(gpu):
    kk, be = gpu
    mc.check_empty(kk, be)


def test_galerkin_product_structure_equals_the_coarse_graph(gpu):
    """A = the 27-point 40^3 lattice with unit values, P (n x num_aggregates, one 1 per row) from graph_mis2_aggregate's labels,
    R = P^T: the off-diagonal structure of R (A P) through kk.spgemm equals graph_explicit_coarsen(compress), entry for entry.  All
    values are positive, so no entry of the product cancels.  (The lattice is the test's own: the generator's 27-point matrix
    repeats the reference generator's boundary rows, whose structure is not symmetric.)"""
    kk, be = gpu
    g = mc.all_cases(False, ("lat27big",))[0]
    n = g.n
    d = mc.Device(kk, be, g)
    labels, nc = kk.graph_mis2_aggregate(d.rm, d.ent)
    lab = be.to_numpy(labels)
    assert np.array_equal(lab, mc.reference(g, "aggregate").labels)
    A = kk.CrsMatrix.from_host(n, n, g.row_map, g.entries, np.ones(g.nnz))
    P = kk.CrsMatrix.from_host(n, nc, np.arange(n + 1), lab, np.ones(n))
    order = np.argsort(lab, kind="stable")
    prm = np.zeros(nc + 1, np.int64)
    np.cumsum(np.bincount(lab, minlength=nc), out=prm[1:])
    R = kk.CrsMatrix.from_host(nc, n, prm, order.astype(np.int32), np.ones(n))
    RAP = kk.spgemm(R, False, kk.spgemm(A, False, P, False), False)
    crm, cent, val = RAP.to_host()
    assert (val > 0).all()
    rows = np.repeat(np.arange(nc), np.diff(crm))
    off = rows != cent
    pairs = np.stack([rows[off], cent[off]], axis=1)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    grm, gent = kk.graph_explicit_coarsen(d.rm, d.ent, labels, nc, True)
    grm, gent = be.to_numpy(grm), be.to_numpy(gent)
    assert gent.size > 0 and np.array_equal(np.bincount(pairs[:, 0], minlength=nc), np.diff(grm))
    assert np.array_equal(pairs[:, 1], gent)
