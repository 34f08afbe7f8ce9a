"""Cases and checks of KokkosSparse::Experimental::spgemm_jacobi, C = B - omega D^-1 (A B), shared by tests/test_emu_spgemm_jacobi.py (SIMT
emulator) and tests/test_gpu_spgemm_jacobi.py (the product library).

The definition.  Row i of A+ is the entry (i, 1) followed by mult_i * A_i, mult_i = -omega * dinv_i, so that C = A+ * B; A+ is not merged
(a row of A that stores its diagonal holds column i twice), which parity_cases.ProductsOf supports: every entry of C is the np.longdouble
sum of its expanded products, b_ik among them.  The structure of A+ * B is pattern(A B) joined with the rows of B -- pattern(A B) itself
exactly when the call's pattern requirement holds, so comparing structures checks the requirement too.

Exact cases.  b = value_bits(n_max + 1, value type): with every value of A+ and of B an integer below 2^b times 2^-4, every partial sum of
an entry, in any order, is representable (parity_cases.value_bits).  The values of A+ are 1 = 16 * 2^-4 and mult_i * a_ij.  omega is one
of 0.5, -2, 1 and dinv_i = +-2^e / |omega| with e in 0..2 drawn per row, a signed power of two: mult_i = +-2^e, so a_ij is drawn with
b - 2 bits and mult_i * a_ij has at most b.  `==` then holds whatever the order in which the library sums, and whenever b_ik joins.

Rounded cases.  Uniform values, omega = 2/3, dinv = 1 / diagonal.  (a) Bit for bit, the documented composition: numpy computes
mult_i = fl(-w * dinv_i) and a'_ij = fl(a_ij * mult_i) in the value type, kkamd_spgemm_numeric multiplies (A', B) on a second handle with the
same settings, numpy adds the stored entries of B in stored order.  (b) |c - exact| <= gamma_(n_ik + 3) (|b_ik| + sum |a_ij mult_i b_jk|),
gamma_r = r u / (1 - r u): an entry with n_ik products takes three roundings in each (mult_i, a'_ij, the product), at most n_ik - 1 in the
sum and one in the last addition, n_ik + 3 on any path; the right side is evaluated in np.longdouble, whose own error (the same expression
with its unit roundoff) is added as parity_cases' bound mode adds it."""
import numpy as np

import oracle
import parity_cases as pc

OMEGAS = (0.5, -2.0, 1.0)
TYPE_GRID = ((np.int32, np.float64), (np.int64, np.float32), (np.int64, np.float64), (np.int32, np.float32))
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
_UINT = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}


def lanes_rule(nnz_b, n):
    """lanes per row of B in the fast epilogue: the smallest power of two, 1..64, that leaves about four entries of the mean row to a lane"""
    want = -(-nnz_b // (4 * n)) if n > 0 else 1
    lanes = 1
    while lanes < 64 and lanes < want:
        lanes *= 2
    return lanes


def strictly_ascending(B0):
    """every row of B0 ascends strictly: what selects the fast form of the epilogue.  (The 27-point lattice of the reference's generator
    does not: its boundary rows store a column twice.)"""
    if B0.nnz < 2:
        return True
    up = np.diff(B0.entries.astype(np.int64)) > 0
    up[B0.row_map[1:-1][(B0.row_map[1:-1] > 0) & (B0.row_map[1:-1] < B0.nnz)] - 1] = True
    return bool(up.all())


def with_diagonal(A0):
    """A0's structure joined with the diagonal, rows sorted, no column twice (values: ones; the checks draw their own)"""
    n = A0.nrows
    rows = np.concatenate([np.repeat(np.arange(n, dtype=np.int64), np.diff(A0.row_map)), np.arange(n, dtype=np.int64)])
    cols = np.concatenate([A0.entries.astype(np.int64), np.arange(n, dtype=np.int64)])
    key = np.unique(rows * A0.ncols + cols)
    rm = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // A0.ncols, minlength=n), out=rm[1:])
    return oracle.Crs(n, A0.ncols, rm, (key % A0.ncols).astype(np.int32), np.ones(len(key)))


def append_diagonal(A0):
    """A0 with (i, i) appended to every row: rows stay unsorted and may hold the diagonal twice"""
    n = A0.nrows
    lens = np.diff(A0.row_map) + 1
    rm = np.zeros(n + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
    ent = np.empty(int(rm[-1]), dtype=np.int32)
    last = rm[1:] - 1
    keep = np.ones(len(ent), dtype=bool); keep[last] = False
    ent[keep] = A0.entries; ent[last] = np.arange(n)
    return oracle.Crs(n, A0.ncols, rm, ent, np.ones(len(ent)))


def diagonal_matrix(n):
    return oracle.Crs(n, n, np.arange(n + 1), np.arange(n, dtype=np.int32), np.ones(n))


def lattice7(nx):
    """the 7-point Laplacian of the nx^3 lattice: 6 on the diagonal, -1 to every neighbour, a symmetric graph with its diagonal stored
    (mis2_cases.lattice; the oracle's generator writes boundary rows the aggregation cannot take: its graph is not symmetric)"""
    import mis2_cases as mc
    g = mc.lattice("lat7", (nx, nx, nx), False)
    rows = np.repeat(np.arange(g.n), np.diff(g.row_map))
    return oracle.Crs(g.n, g.n, g.row_map, g.entries, np.where(g.entries == rows, 6.0, -1.0))


def tentative_prolongator(kk, be, A0):
    """one unit entry per row, at the row's MIS-2 aggregate (graph_mis2_aggregate on A's graph): (P_tent, labels, aggregates)"""
    labels, nagg = kk.graph_mis2_aggregate(be.from_numpy(A0.row_map.astype(np.int32)), be.from_numpy(A0.entries), backend=be)
    labels = np.asarray(be.to_numpy(labels)).astype(np.int32)
    assert labels.min() == 0 and labels.max() == nagg - 1 and 1 < nagg < A0.nrows
    return oracle.Crs(A0.nrows, int(nagg), np.arange(A0.nrows + 1), labels, np.ones(A0.nrows)), labels, int(nagg)


def rows_of_lengths(lens, ncols, seed):
    """a matrix whose row i holds lens[i] distinct ascending columns"""
    rng = np.random.default_rng(seed)
    rm = np.zeros(len(lens) + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
    ent = np.concatenate([np.sort(rng.choice(ncols, size=int(l), replace=False)) for l in lens] + [np.zeros(0, dtype=np.int64)]).astype(np.int32)
    return oracle.Crs(len(lens), ncols, rm, ent, np.ones(len(ent)))


def width_operands(lanes):
    """(A, B): A diagonal, B with rows of 0, 1, lanes - 1, lanes, lanes + 1, 65 and 300 entries and as many rows of 3 lanes entries as it takes
    for the rule to choose `lanes`"""
    special = [0, 1, max(lanes - 1, 0), lanes, lanes + 1, 65, 300]
    fill = 0
    while lanes_rule(sum(special) + 3 * lanes * fill, len(special) + fill) != lanes:
        fill += 1
        assert fill < 4000
    lens = np.array(special + [3 * lanes] * fill)
    lens = lens[np.random.default_rng(lanes).permutation(len(lens))]
    B0 = rows_of_lengths(lens, 400, seed=100 + lanes)
    assert lanes_rule(B0.nnz, B0.nrows) == lanes
    return diagonal_matrix(B0.nrows), B0


C_ROW_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)


def bisection_operands():
    """rows of C of every length in C_ROW_LENGTHS, twice: row i < R of A holds (i, i) and (i, R + i), row R + i of B the columns 10 .. 10 + length
    and row i of B one of them, the first (even i) or the last (odd i); rows R + i of A are diagonal"""
    lens = [l for l in C_ROW_LENGTHS for _ in (0, 1)]
    R = len(lens)
    a_rm = np.concatenate([2 * np.arange(R), 2 * R + np.arange(R + 1)])
    a_ent = np.concatenate([np.stack([np.arange(R), R + np.arange(R)], axis=1).ravel(), R + np.arange(R)]).astype(np.int32)
    A0 = oracle.Crs(2 * R, 2 * R, a_rm, a_ent, np.ones(len(a_ent)))
    b_lens = np.concatenate([np.ones(R, dtype=np.int64), np.array(lens)])
    b_rm = np.zeros(2 * R + 1, dtype=np.int64); np.cumsum(b_lens, out=b_rm[1:])
    short = [10 if i % 2 == 0 else 10 + lens[i] - 1 for i in range(R)]
    b_ent = np.concatenate([np.array(short)] + [10 + np.arange(l) for l in lens]).astype(np.int32)
    B0 = oracle.Crs(2 * R, 10 + max(lens) + 5, b_rm, b_ent, np.ones(len(b_ent)))
    return A0, B0, np.array(lens)


def unsorted_with_repeats(n, k, seed):
    """rows in random order that hold some column twice"""
    B0 = oracle.random_crs(n, k, 9, variance=5, seed=seed)
    assert (np.diff(B0.row_map) >= 2).any()
    ent = B0.entries.copy()
    for i in range(0, n, 3):                                       # every third row repeats its first column at its end
        lo, hi = B0.row_map[i], B0.row_map[i + 1]
        if hi - lo >= 2:
            ent[hi - 1] = ent[lo]
    return oracle.Crs(n, k, B0.row_map, ent, np.ones(B0.nnz))


def exact_operands(kk, be):
    """name -> (A, B) of check 1; the MIS-2 prolongator comes from the library under test"""
    L27 = oracle.laplace3d("FE", 6, 5, 4)
    L7 = lattice7(8)
    R = with_diagonal(oracle.rmat(9, 8))
    G = append_diagonal(oracle.random_crs(300, 300, 7, variance=3, seed=21))
    D = diagonal_matrix(257)
    return {"lat27_squared": (L27, L27), "lat7_prolongator": (L7, tentative_prolongator(kk, be, L7)[0]), "rmat_squared": (R, R),
            "unsorted_B": (G, unsorted_with_repeats(300, 280, seed=22)), "diagonal_A": (D, rows_of_lengths(np.arange(257) % 23, 300, seed=23))}


# ---------------------------------------------------------------------------------------------------------------- the definition
class Definition:
    """C = A+ * B of the module's header for one pair of structures: products, structure, which entries lie on B's pattern, n_ik"""

    def __init__(self, A0, B0, row0=0):
        assert A0.ncols == B0.nrows
        m = A0.nrows
        lens = np.diff(A0.row_map) + 1
        rm = np.zeros(m + 1, dtype=np.int64); np.cumsum(lens, out=rm[1:])
        first = rm[:-1]
        self.unit = np.zeros(int(rm[-1]), dtype=bool); self.unit[first] = True
        ent = np.empty(int(rm[-1]), dtype=np.int32)
        ent[self.unit] = row0 + np.arange(m); ent[~self.unit] = A0.entries
        self.row_of = np.repeat(np.arange(m), np.diff(A0.row_map))
        self.plus = oracle.Crs(m, A0.ncols, rm, ent, None)
        self.P = pc.ProductsOf(self.plus, B0)
        on_b = np.zeros(len(self.P.a_idx), dtype=np.int64); on_b[self.unit[self.P.a_idx]] = 1
        self.copies = np.add.reduceat(on_b, self.P.first) if self.P.first.size else np.zeros(0, dtype=np.int64)      # stored copies of (i, k) in B's row
        self.n_ab = self.P.n - self.copies
        self.nnz = int(self.P.row_map[-1])

    def values_plus(self, va, mult):
        """the values of A+ in np.longdouble: 1, then mult_i * a_ij (one exact product when both are powers of two times integers)"""
        v = np.empty(len(self.unit), dtype=np.longdouble)
        v[self.unit] = 1
        with np.errstate(invalid="ignore", over="ignore"):
            v[~self.unit] = va.astype(np.longdouble) * mult.astype(np.longdouble)[self.row_of]
        return v

    def reduce(self, va, mult, vb):
        return self.P.reduce(self.values_plus(va, mult), vb)


def same_bits_or_nan(a, b):
    u = _UINT[np.dtype(a.dtype)]
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


class Call:
    """one handle, A and B on the device, C from the symbolic phase; jacobi() and numeric() may be repeated with new values"""

    def __init__(self, kk, be, A0, B0, odt, vdt, verbose=False):
        self.kk, self.be, self.A0, self.B0, self.odt, self.vdt = kk, be, A0, B0, odt, np.dtype(vdt)
        self.kh = kk.KokkosKernelsHandle(be)
        self.kh.create_spgemm_handle("SPGEMM_KK")
        self.sh = self.kh.get_spgemm_handle()
        if verbose:
            self.sh.set("verbose", 1)
        self.A = pc.dev(be, pc._with_values(A0, np.ones(A0.nnz)), odt, vdt)
        self.B = pc.dev(be, pc._with_values(B0, np.ones(B0.nnz)), odt, vdt)
        self.Cm = kk.spgemm_symbolic(self.kh, self.A, False, self.B, False)

    def _operands(self, va, vb):
        kk, be = self.kk, self.be
        A = kk.CrsMatrix(self.A0.nrows, self.A0.ncols, self.A.graph.row_map, self.A.graph.entries, be.from_numpy(np.asarray(va).astype(self.vdt)), backend=be)
        B = kk.CrsMatrix(self.B0.nrows, self.B0.ncols, self.B.graph.row_map, self.B.graph.entries, be.from_numpy(np.asarray(vb).astype(self.vdt)), backend=be)
        return A, B

    def jacobi(self, va, vb, omega, dinv):
        A, B = self._operands(va, vb)
        self.kk.spgemm_jacobi(self.kh, A, False, B, False, self.Cm, omega, None if dinv is None else self.be.from_numpy(np.asarray(dinv).astype(self.vdt)))
        return self.host()

    def numeric(self, va, vb):
        A, B = self._operands(va, vb)
        self.kk.spgemm_numeric(self.kh, A, False, B, False, self.Cm)
        return self.host()

    def host(self):
        rm, ent, val = self.Cm.to_host()
        nnz = int(rm[-1]) if len(rm) else 0
        return np.asarray(rm).astype(np.int64), np.asarray(ent)[:nnz], np.asarray(val)[:nnz]

    def form(self):
        return self.sh.get(24), self.sh.get(25)


def draw_exact(rng, D, B0, A0, vdt, omega):
    b = pc.value_bits(D.P.n_max + 1, vdt)
    assert b - 2 >= (11 if np.dtype(vdt) == np.float64 else 3) and b >= 5, "%d products meet in one entry: %d-bit values cannot tell a rounding apart" % (D.P.n_max, b)
    va, vb = pc.exact_values(rng, A0.nnz, b - 2), pc.exact_values(rng, B0.nnz, b)
    dinv = np.where(rng.random(A0.nrows) < 0.5, -1.0, 1.0) * 2.0 ** rng.integers(0, 3, size=A0.nrows) / abs(omega)
    return va, vb, dinv


def assert_structure(D, rm, ent, name):
    assert np.array_equal(rm, D.P.row_map), name + ": row_map differs from the definition's"
    assert np.array_equal(ent, D.P.entries), name + ": entries differ (rows of C must leave column-sorted)"


def compare_with_definition(D, got, va, mult, vb, name, special=False):
    sums, _ = D.reduce(va, mult, vb)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = sums.astype(np.float64)
    got = got.astype(np.float64)
    nan = np.isnan(ref)
    if not special:
        assert (ref == sums).all() and not nan.any(), name + ": the definition's sums are not representable (the case's bits are wrong)"
    assert np.array_equal(np.isnan(got), nan), name + ": NaN at other entries than the definition's"
    bad = ~nan & (got != ref)
    if bad.any():
        i = int(np.flatnonzero(bad)[0]); r = int(np.searchsorted(D.P.row_map, i, side="right") - 1)
        raise AssertionError("%s: %d values differ, first at row %d column %d (%d products, %d copies in B): %r, definition %r"
                             % (name, int(bad.sum()), r, int(D.P.entries[i]), int(D.n_ab[i]), int(D.copies[i]), got[i], ref[i]))
    return ref


def check_exact(kk, be, name, A0, B0, odt, vdt, seed=0, expect_fast=None):
    """check 1: structure and values `==` the definition, for omega in OMEGAS on one handle (every call after the first is a reuse: new values,
    another omega, another dinv, entries(C) kept)"""
    D = Definition(A0, B0)
    rng = np.random.default_rng([seed, 5])
    call = Call(kk, be, A0, B0, odt, vdt)
    for rnd, omega in enumerate(OMEGAS):
        va, vb, dinv = draw_exact(rng, D, B0, A0, vdt, omega)
        rm, ent, val = call.jacobi(va, vb, omega, dinv)
        tag = "%s %s/%s omega=%g" % (name, np.dtype(odt).name, np.dtype(vdt).name, omega)
        assert_structure(D, rm, ent, tag)
        compare_with_definition(D, val, va, -omega * dinv, vb, tag)
        lanes, fast = call.form()
        assert fast == int(strictly_ascending(B0)), tag
        if expect_fast is not None:
            assert fast == int(expect_fast), tag
        assert lanes == (lanes_rule(B0.nnz, B0.nrows) if fast else 1), (tag, lanes)
    return call


def composition(call, va, vb, omega, dinv):
    """the documented composition: A' in the value type by numpy, N = kkamd_spgemm_numeric(A', B) on a second handle with the same settings,
    then numpy's additions of B's stored entries in the value type, in stored order"""
    vdt, A0, B0 = call.vdt, call.A0, call.B0
    with np.errstate(invalid="ignore", over="ignore"):
        mult = (-vdt.type(omega)) * np.asarray(dinv).astype(vdt)
        assert mult.dtype == vdt
        va2 = np.asarray(va).astype(vdt) * np.repeat(mult, np.diff(A0.row_map))
    second = Call(call.kk, call.be, A0, B0, call.odt, vdt)
    rm, ent, val = second.numeric(va2, vb)
    val = val.copy()
    assert val.dtype == vdt
    rows = np.repeat(np.arange(B0.nrows), np.diff(B0.row_map))[:B0.row_map[A0.nrows]]
    key_c = np.repeat(np.arange(A0.nrows, dtype=np.int64), np.diff(rm)) * B0.ncols + ent
    pos = np.searchsorted(key_c, rows.astype(np.int64) * B0.ncols + B0.entries[:len(rows)])
    assert (pos < len(key_c)).all() and np.array_equal(key_c[pos], rows.astype(np.int64) * B0.ncols + B0.entries[:len(rows)])
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(val, pos, np.asarray(vb).astype(vdt)[:len(rows)])          # unbuffered, in index order: repeated columns one after another
    return rm, ent, val


def draw_rounded(rng, A0, B0, vdt):
    va = rng.uniform(-50, 50, A0.nnz).astype(vdt).astype(np.float64)
    vb = rng.uniform(-50, 50, B0.nnz).astype(vdt).astype(np.float64)
    diag = rng.uniform(1, 50, A0.nrows) * np.where(rng.random(A0.nrows) < 0.5, -1.0, 1.0)
    rows = np.repeat(np.arange(A0.nrows), np.diff(A0.row_map))
    on = A0.entries == rows
    va[on] = diag[rows[on]].astype(vdt).astype(np.float64)
    dinv = (vdt.type(1) / diag.astype(vdt)).astype(np.float64)
    return va, vb, dinv


def check_rounded(kk, be, name, A0, B0, odt, vdt, seed=0, capfd=None):
    """checks 2 and 3 on the same inputs; returns (the largest share of the bound used, whether check 2 compared bits).

    Check 2 needs N = kkamd_spgemm_numeric(A', B) to be the same bits in two calls.  It is where one wave owns a row's accumulator (the
    value kernels "quad" and "wave": one instruction stream, and the hardware serves the lanes of one LDS add in a fixed order).  The other
    value kernels add into one table from several waves with floating-point atomics, in the order the waves arrive: two numeric calls on
    the same operands then differ in last bits (on the MI355X, R-MAT squared: hundreds of entries), so no composition can be compared bit
    for bit with them.  With capfd the library's verbose line says which kernels took rows; bits are compared when only those two did,
    otherwise the numbers of differing entries (result against composition, composition against a second composition) are printed and
    the bound alone is asserted.  Without capfd (the emulator runs work-items one after another) bits are always compared."""
    vdt = np.dtype(vdt)
    rng = np.random.default_rng([seed, 9])
    omega = 2.0 / 3.0
    va, vb, dinv = draw_rounded(rng, A0, B0, vdt)
    call = Call(kk, be, A0, B0, odt, vdt)
    one_wave = True
    if capfd is not None:
        capfd.readouterr(); call.sh.set("verbose", 1)
    rm, ent, val = call.jacobi(va, vb, omega, dinv)
    if capfd is not None:
        call.sh.set("verbose", 0)
        _, kernels = pc.parse_numeric_verbose(capfd.readouterr().out)
        one_wave = sum(kernels[k_] for k_ in pc.VALUE_KERNELS if k_ not in ("quad", "wave")) == 0
    tag = "%s %s/%s" % (name, np.dtype(odt).name, vdt.name)
    D = Definition(A0, B0)
    assert_structure(D, rm, ent, tag)
    rm2, ent2, val2 = composition(call, va, vb, omega, dinv)
    assert np.array_equal(rm2, rm) and np.array_equal(ent2, ent)
    u_t = _UINT[vdt]
    bad = val.view(u_t) != val2.view(u_t)
    if one_wave:
        assert not bad.any(), "%s: %d values differ from the documented composition, first at entry %d: %r, composition %r" % (
            tag, int(bad.sum()), int(np.flatnonzero(bad)[0]), val[np.flatnonzero(bad)[0]], val2[np.flatnonzero(bad)[0]])
    else:
        _, _, val3 = composition(call, va, vb, omega, dinv)
        print("%s: several waves share accumulators: %d of %d entries differ from the composition in bits, %d between two compositions"
              % (tag, int(bad.sum()), len(val), int((val2.view(u_t) != val3.view(u_t)).sum())))
    # the bound: mult as the library rounds it is within the three roundings counted per product, so the exact side uses the unrounded one
    w = np.longdouble(vdt.type(omega))
    sums, S = D.reduce(va, np.asarray(-w * dinv.astype(np.longdouble)), vb)
    u = pc.U_ROUND[vdt]; ul = float(np.finfo(np.longdouble).eps) / 2
    r = (D.n_ab + 3).astype(np.longdouble)
    bound = (r * u / (1 - r * u) + r * ul / (1 - r * ul)) * S
    err = np.abs(val.astype(np.longdouble) - sums)
    share = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print("%s: largest share of the bound gamma_(n+3) S used: %.3f" % (tag, share))
    badb = ~(err <= bound)
    assert not badb.any(), "%s: %d entries outside the bound, first %d: error %r, bound %r" % (
        tag, int(badb.sum()), int(np.flatnonzero(badb)[0]), err[np.flatnonzero(badb)[0]], bound[np.flatnonzero(badb)[0]])
    return share, one_wave


def check_widths(kk, be, lanes, odt, vdt):
    """check 4, rows of B: every special length under every width the rule can choose; query 24 says the width ran"""
    A0, B0 = width_operands(lanes)
    call = check_exact(kk, be, "width%d" % lanes, A0, B0, odt, vdt, seed=lanes, expect_fast=True)
    assert call.form() == (lanes, 1)


def check_bisection(kk, be, odt, vdt):
    """check 4, rows of C: lengths around every power of two, B's column at the first and at the last entry"""
    A0, B0, lens = bisection_operands()
    call = check_exact(kk, be, "bisection", A0, B0, odt, vdt, seed=3, expect_fast=True)
    rm, _, _ = call.host()
    assert np.array_equal(np.diff(rm)[:len(lens)], lens) and set(C_ROW_LENGTHS) <= set(np.diff(rm).tolist())


def check_forms(kk, be):
    """query 25: 1 for sorted B, 0 for the unsorted one (one lane per row then), and for a sorted B that repeats a column"""
    ops = exact_operands(kk, be)
    assert check_exact(kk, be, "sorted", *ops["rmat_squared"], np.int32, np.float64, expect_fast=True).form()[1] == 1
    assert check_exact(kk, be, "unsorted", *ops["unsorted_B"], np.int32, np.float64, expect_fast=False).form() == (1, 0)
    A0 = diagonal_matrix(40)
    B0 = oracle.Crs(40, 50, 3 * np.arange(41), np.tile(np.array([4, 9, 9], dtype=np.int32), 40), np.ones(120))     # ascending, not strictly
    assert check_exact(kk, be, "repeats", A0, B0, np.int64, np.float32, expect_fast=False).form() == (1, 0)


def check_empty(kk, be):
    """m = 0, c_nnz = 0 (B without entries; A without entries and B with: the pattern requirement fails)"""
    for odt in (np.int32, np.int64):
        E = oracle.Crs(0, 0, np.zeros(1), np.zeros(0), np.zeros(0))
        call = Call(kk, be, E, E, odt, np.float64)
        rm, ent, val = call.jacobi(np.zeros(0), np.zeros(0), 1.0, np.zeros(0))
        assert len(ent) == 0 and len(val) == 0
        A0 = diagonal_matrix(12)
        B0 = oracle.Crs(12, 9, np.zeros(13), np.zeros(0), np.zeros(0))
        call = Call(kk, be, A0, B0, odt, np.float32)
        assert call.sh.get(0) == 0
        rm, ent, val = call.jacobi(np.ones(12), np.zeros(0), 0.5, np.ones(12))
        assert not rm.any() and len(val) == 0
        call.jacobi(np.ones(12), np.zeros(0), 0.5, None)                       # a null dinv is an error only with c_nnz > 0
        A1 = oracle.Crs(12, 12, np.zeros(13), np.zeros(0), np.zeros(0))
        B1 = rows_of_lengths([0, 0, 0, 2] + [1] * 8, 9, seed=1)
        call = Call(kk, be, A1, B1, odt, np.float64)
        assert call.sh.get(0) == 0
        try:
            call.jacobi(np.zeros(0), np.ones(B1.nnz), 0.5, np.ones(12))
        except kk.KkamdError as e:
            assert e.status == kk._capi.ERR_INVALID_ARG and "row 3 " in str(e), str(e)
        else:
            raise AssertionError("an empty A * B cannot hold the rows of B")


def check_special(kk, be, odt, vdt):
    """check 5: dinv_i = Inf in one row, NaN in one entry of B; omega = 0"""
    vdt = np.dtype(vdt)
    A0 = oracle.laplace3d("FE", 6, 5, 4)
    D = Definition(A0, A0)
    rng = np.random.default_rng(77)
    va, vb, dinv = draw_exact(rng, D, A0, A0, vdt, 0.5)
    row_inf, ent_nan = 17, int(A0.row_map[40]) + 2
    dinv[row_inf] = np.inf
    vb[ent_nan] = np.nan
    call = Call(kk, be, A0, A0, odt, vdt)
    rm, ent, val = call.jacobi(va, vb, 0.5, dinv)
    assert_structure(D, rm, ent, "special")
    with np.errstate(invalid="ignore"):
        ref = compare_with_definition(D, val, va, -0.5 * dinv, vb, "special", special=True)
    rows = np.repeat(np.arange(A0.nrows), np.diff(rm))
    assert not np.isfinite(ref[rows == row_inf]).any() and np.isnan(ref).any() and np.isfinite(ref[rows != row_inf]).sum() > len(ref) // 2
    # NaN exactly where a product or a copy of B's entry (40, column) reaches: rows with a_i,40 stored, at that column
    col_nan = int(A0.entries[ent_nan])
    reach = np.zeros(A0.nrows, dtype=bool)
    reach[np.repeat(np.arange(A0.nrows), np.diff(A0.row_map))[A0.entries == 40]] = True
    want_nan = (reach[rows] & (ent == col_nan))
    assert np.array_equal(np.isnan(val[rows != row_inf]), want_nan[rows != row_inf])
    _, _, comp = composition(call, va, vb, 0.5, dinv)
    assert same_bits_or_nan(val, comp).all(), "special values: differs from the documented composition"
    # omega = 0: b_ik on B's pattern, signed zeros elsewhere, no shortcut (the composition says which zero)
    va, vb, dinv = draw_exact(rng, D, A0, A0, vdt, 1.0)
    rm, ent, val = call.jacobi(va, vb, 0.0, dinv)
    on_b = D.copies > 0
    sums, _ = D.P.reduce(np.where(D.unit, 1.0, 0.0), vb)
    assert np.array_equal(val[on_b].astype(np.float64), sums[on_b].astype(np.float64)) and (val[~on_b] == 0).all() and (~on_b).any()
    _, _, comp = composition(call, va, vb, 0.0, dinv)
    assert same_bits_or_nan(val, comp).all(), "omega = 0: differs from the documented composition"


def _status(kk, fn):
    try:
        fn()
    except kk.KkamdError as e:
        return e.status, str(e)
    except ValueError as e:                                    # KKAMD_ERR_STATE through the Python interface
        return kk._capi.ERR_STATE, str(e)
    return kk._capi.OK, ""


def check_statuses(kk, be):
    """check 6"""
    lib, capi = be.lib, kk._capi
    A0 = oracle.laplace3d("FD", 4, 3, 3)
    n = A0.nrows
    A = pc.dev(be, A0)
    kh = kk.KokkosKernelsHandle(be); kh.create_spgemm_handle()
    sh = kh.get_spgemm_handle()
    Cfake = kk.CrsMatrix(n, n, be.empty(n + 1, np.int32), be.empty(1, np.int32), be.empty(1, np.float64), backend=be)
    ones = be.from_numpy(np.ones(n))
    st, msg = _status(kk, lambda: kk.spgemm_jacobi(kh, A, False, A, False, Cfake, 1.0, ones))
    assert st == capi.ERR_STATE and "must first call spgemm_symbolic" in msg, (st, msg)
    assert lib.kkamd_spgemm_jacobi(None, 1, 1, 1, None, None, None, None, None, None, None, None, None, 1.0, None, 0, 1, None) == capi.ERR_STATE
    Cm = kk.spgemm_symbolic(kh, A, False, A, False)
    st, msg = _status(kk, lambda: kk.spgemm_jacobi(kh, A, False, A, False, Cm, 1.0, None))
    assert st == capi.ERR_INVALID_ARG and "dinv" in msg, (st, msg)
    args = [be.ptr(A.graph.row_map), be.ptr(A.graph.entries), be.ptr(A.values)] * 2 + [be.ptr(Cm.graph.row_map), be.ptr(Cm.graph.entries), be.ptr(Cm.values)]
    assert lib.kkamd_spgemm_jacobi(sh.h, n, n, n, *args, 1.0, be.ptr(ones), 0, 7, be.stream()) == capi.ERR_UNSUPPORTED
    assert lib.kkamd_spgemm_jacobi(sh.h, n, n, n + 1, *args, 1.0, be.ptr(ones), 0, 1, be.stream()) == capi.ERR_STATE
    with np.testing.assert_raises(RuntimeError):
        kk.spgemm_jacobi(kh, A, True, A, False, Cm, 1.0, ones)
    # m != n
    R0 = oracle.random_crs(5, 8, 3, seed=1, sorted_rows=True); S0 = oracle.random_crs(8, 6, 3, seed=2, sorted_rows=True)
    kh2 = kk.KokkosKernelsHandle(be); kh2.create_spgemm_handle()
    Rd, Sd = pc.dev(be, R0), pc.dev(be, S0)
    C2 = kk.spgemm_symbolic(kh2, Rd, False, Sd, False)
    st, msg = _status(kk, lambda: kk.spgemm_jacobi(kh2, Rd, False, Sd, False, C2, 1.0, be.from_numpy(np.ones(5))))
    assert st == capi.ERR_INVALID_ARG and "square" in msg, (st, msg)
    # no diagonal: A = [[., 1], [1, .]], B = I -- the row of B is not in the row of A * B
    X0 = oracle.Crs(2, 2, [0, 1, 2], [1, 0], [1.0, 1.0]); I0 = diagonal_matrix(2)
    call = Call(kk, be, X0, I0, np.int32, np.float64)
    st, msg = _status(kk, lambda: call.jacobi(np.ones(2), np.ones(2), 1.0, np.ones(2)))
    assert st == capi.ERR_INVALID_ARG and "row 0 " in msg, (st, msg)
    # ... and a correct call on the same handle succeeds afterwards: the same A against a B whose rows are inside A * B
    call2 = Call(kk, be, X0, I0, np.int32, np.float64)
    _status(kk, lambda: call2.jacobi(np.ones(2), np.ones(2), 1.0, np.ones(2)))
    Y0 = oracle.Crs(2, 2, [0, 2, 4], [0, 1, 0, 1], np.ones(4))
    held = (call2.A, call2.B, call2.Cm)                       # alive, so that no new array takes an address the handle has seen
    call2.A0, call2.B0 = Y0, Y0
    call2.A = call2.B = pc.dev(be, Y0)
    call2.Cm = kk.spgemm_symbolic(call2.kh, call2.A, False, call2.B, False)
    D = Definition(Y0, Y0)
    va = np.array([2.0, -3.0, 0.5, 4.0])
    rm, ent, val = call2.jacobi(va, va, 0.5, np.array([2.0, -4.0]))
    assert_structure(D, rm, ent, "after an error")
    compare_with_definition(D, val, va, -0.5 * np.array([2.0, -4.0]), va, "after an error")
    del held


def check_dist(kk, be, odt=np.int32, vdt=np.float64):
    """check 7: world 2, both ranks in turn in this process, kkamd_dist_spgemm_partition's offsets on the exact-valued R-MAT case: the two slabs
    concatenated `==` the one-GPU C"""
    from kokkos_kernels_amd import dist
    A0 = with_diagonal(oracle.rmat(9, 8))
    D = Definition(A0, A0)
    rng = np.random.default_rng(31)
    va, vb, dinv = draw_exact(rng, D, A0, A0, vdt, -2.0)
    call = Call(kk, be, A0, A0, odt, vdt)
    rm, ent, val = call.jacobi(va, vb, -2.0, dinv)
    compare_with_definition(D, val, va, 2.0 * dinv, vb, "one GPU")
    Bd = pc.dev(be, pc._with_values(A0, vb), odt, vdt)
    offs, _ = dist.DistSpgemm.partition(pc.dev(be, pc._with_values(A0, va), odt, vdt), Bd, 2)
    assert offs[0] == 0 and offs[2] == A0.nrows and 0 < offs[1] < A0.nrows, offs
    parts = []
    for rank in range(2):
        lo, hi = offs[rank], offs[rank + 1]
        e0, e1 = int(A0.row_map[lo]), int(A0.row_map[hi])
        slab = oracle.Crs(hi - lo, A0.ncols, A0.row_map[lo:hi + 1] - e0, A0.entries[e0:e1], va[e0:e1])
        As = pc.dev(be, slab, odt, vdt)
        op = dist.DistSpgemm(offs, rank, be)
        Cs = op.symbolic(As, Bd)
        op.jacobi(As, Bd, Cs, -2.0, be.from_numpy(dinv[lo:hi].astype(vdt)))
        r, e, v = Cs.to_host()
        parts.append((np.asarray(r).astype(np.int64), np.asarray(e), np.asarray(v)))
    assert np.array_equal(np.concatenate([parts[0][0], parts[1][0][1:] + parts[0][0][-1]]), rm)
    assert np.array_equal(np.concatenate([parts[0][1], parts[1][1]])[:len(ent)], ent)
    assert np.array_equal(np.concatenate([parts[0][2], parts[1][2]])[:len(val)], val)
    # a partition of another size than A's columns is refused
    op = dist.DistSpgemm([0, 3, 5], 0, be)
    R0 = oracle.random_crs(3, 8, 3, seed=1, sorted_rows=True); S0 = oracle.random_crs(8, 6, 3, seed=2, sorted_rows=True)
    Rd, Sd = pc.dev(be, R0, odt, vdt), pc.dev(be, S0, odt, vdt)
    Cs = op.symbolic(Rd, Sd)
    st, msg = _status(kk, lambda: op.jacobi(Rd, Sd, Cs, 1.0, be.from_numpy(np.ones(3, dtype=vdt))))
    assert st == kk._capi.ERR_INVALID_ARG and "square" in msg, (st, msg)


def check_use(kk, be, vdt=np.float64):
    """check 8: the smoothed prolongator P = (I - omega D^-1 A) P_tent of the 7-point 12^3 lattice"""
    vdt = np.dtype(vdt)
    A0 = lattice7(12)
    P0, labels, nagg = tentative_prolongator(kk, be, A0)
    rows = np.repeat(np.arange(A0.nrows), np.diff(A0.row_map))
    diag = np.zeros(A0.nrows); diag[rows[A0.entries == rows]] = A0.values[A0.entries == rows]
    assert (diag != 0).all()
    omega = 2.0 / 3.0
    dinv = (vdt.type(1) / diag.astype(vdt)).astype(np.float64)
    call = Call(kk, be, A0, P0, np.int32, vdt)
    rm, ent, val = call.jacobi(A0.values, P0.values, omega, dinv)
    for i in range(A0.nrows):                                  # row i: exactly the labels of the closed neighbourhood of i
        nb = A0.entries[A0.row_map[i]:A0.row_map[i + 1]]
        assert np.array_equal(ent[rm[i]:rm[i + 1]], np.unique(labels[nb])), i
    D = Definition(A0, P0)
    w = np.longdouble(vdt.type(omega))
    _, S = D.reduce(A0.values, np.asarray(-w * dinv.astype(np.longdouble)), P0.values)
    u = pc.U_ROUND[vdt]
    r = (D.n_ab + 3).astype(np.longdouble)
    bound = np.add.reduceat(r * u / (1 - r * u) * S, rm[:-1])
    zero_sum = np.add.reduceat(A0.values, A0.row_map[:-1]) == 0
    assert zero_sum.sum() > A0.nrows // 4
    # 1 / diag is rounded once more than the bound of an entry counts for an exact dinv: the row sum 1 - w dinv_i sum_j a_ij is exactly 1
    # only where sum_j a_ij = 0 exactly, whatever dinv_i is -- so the rounding of dinv does not enter
    row_sum = np.add.reduceat(val.astype(np.longdouble), rm[:-1])
    err = np.abs(row_sum - 1)
    assert (err[zero_sum] <= bound[zero_sum]).all(), (float(err[zero_sum].max()), float(bound[zero_sum].min()))
    print("smoothed prolongator: %d aggregates, %d rows with a zero row sum of A, largest |row sum - 1| / bound = %.3f"
          % (nagg, int(zero_sum.sum()), float((err[zero_sum] / bound[zero_sum]).max())))
    return nagg
