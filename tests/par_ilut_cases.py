"""ParILUT cases shared by the emulator and GPU tests (CPU only, like spiluk_cases.py).

The reference's loop (sparse/impl/KokkosSparse_par_ilut_numeric_impl.hpp:724-876) restated in numpy, step by step, on rows held as
{column: value} dicts in ascending column order, with a dtype parameter (float32, float64, longdouble) and an optional generator that takes
the terms of every dot product, product sum and the residual's sum in a random order.

Whole-loop cases: rounding may decide neither a pattern nor the stop, so analysed() asserts that float32, float64, longdouble and 8 random
term orders each in float32 and float64 give the same patterns of L and U and the same num_iters; a seed that fails is replaced here, no
case is skipped at run time.  The value tolerance of a case and dtype is 4 times the largest deviation of those 8 re-ordered runs and of the
longdouble run from the plain run of that dtype: 8 samples understate the tail of an order-dependent rounding error and the library's tree
order is one more sample of the same population.  analysed() prints the measured spread.

Step cases: small integers with every divisor a power of two, so every operation is exact and any summation order gives the same bits in
float32 and float64 (exact_inputs() asserts it on the CPU).
"""
import ctypes as C
import functools
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REORDERS = 8
MARGIN = 4.0


# ---------------------------------------------------------------- scalars and rows
def scalar(dtype):
    """the constructor of one value: python floats are IEEE doubles (the same bits as numpy.float64, several times faster)"""
    return float if np.dtype(dtype) == np.float64 else np.dtype(dtype).type


def _div(a, b):
    if isinstance(a, float) and isinstance(b, float):
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))
    with np.errstate(all="ignore"):
        return a / b


def _sum(terms, zero, rng):
    if rng is not None and len(terms) > 1:
        terms = [terms[i] for i in rng.permutation(len(terms))]
    acc = zero
    for t in terms:
        acc = acc + t
    return acc


def _sorted(row):
    return dict(sorted(row.items()))


class Csr:
    def __init__(self, n, row_map, entries, values):
        self.n, self.row_map, self.entries, self.values = n, np.asarray(row_map, dtype=np.int64), np.asarray(entries, dtype=np.int32), values

    @classmethod
    def from_rows(cls, rows, dtype=np.float64):
        rm = np.zeros(len(rows) + 1, dtype=np.int64)
        rm[1:] = np.cumsum([len(r) for r in rows])
        ent = np.array([c for r in rows for c in r], dtype=np.int32)
        val = np.array([v for r in rows for v in r.values()], dtype=np.longdouble).astype(dtype)
        return cls(len(rows), rm, ent, val)

    def rows(self, dt=float):
        return [{int(self.entries[p]): dt(self.values[p]) for p in range(self.row_map[i], self.row_map[i + 1])} for i in range(self.n)]

    @property
    def nnz(self):
        return int(self.row_map[-1])


# ---------------------------------------------------------------- the restated steps
def ref_initial(A, dt):
    """initialize_LU (:673-719) on the symbolic pattern (symbolic_impl.hpp:36-93)"""
    L, U = [], []
    for i, r in enumerate(A):
        l = {c: dt(v) for c, v in r.items() if c < i}
        l[i] = dt(1)
        u = {i: dt(r.get(i, 1.0))}
        u.update({c: dt(v) for c, v in r.items() if c > i})
        L.append(l); U.append(u)
    return L, U


def ref_product(L, U, dt, rng=None):
    out = []
    for i in range(len(L)):
        terms = {}
        for k, lv in L[i].items():
            for c, uv in U[k].items():
                terms.setdefault(c, []).append(lv * uv)
        out.append({c: _sum(t, dt(0), rng) for c, t in sorted(terms.items())})
    return out


def ref_add_candidates(A, L, U, LU, dt):
    """:129-328"""
    Ln, Un = [], []
    for i in range(len(A)):
        ln, un = {}, {}
        for c in sorted(set(A[i]) | set(LU[i])):
            r = dt(A[i].get(c, 0.0)) - LU[i].get(c, dt(0))
            if c < i and c in L[i]:
                o = L[i][c]
            elif c >= i and c in U[i]:
                o = U[i][c]
            else:
                o = _div(r, U[c][c]) if c < i else r
            if c <= i:
                ln[c] = dt(1) if c == i else o
            if c >= i:
                un[c] = o
        Ln.append(ln); Un.append(un)
    return Ln, Un


def ref_transpose(U):
    Ut = [{} for _ in U]
    for i, r in enumerate(U):
        for c, v in r.items():
            Ut[c][i] = v
    return Ut


def ref_sweep(A, L, U, Ut, dt, rng=None):
    """compute_l_u_factors with async_update == false (:354-458): in place, Ut frozen"""
    def s(i, c):
        last = min(i, c)
        terms = [lv * Ut[c][k] for k, lv in L[i].items() if k < last and k in Ut[c]]
        return dt(A[i].get(c, 0.0)) - _sum(terms, dt(0), rng)
    for i in range(len(A)):
        for c in list(L[i]):
            if c == i:
                continue
            ud = Ut[c][max(Ut[c])] if Ut[c] else dt(0)
            if ud != 0:
                L[i][c] = _div(s(i, c), ud)
        for c in list(U[i]):
            U[i][c] = s(i, c)


def ref_select(M, rank, dtype):
    """:480-494: the order statistic of |values|"""
    v = np.abs(np.array([x for r in M for x in r.values()], dtype=dtype))
    return v[np.argpartition(v, rank)[rank]] if np.dtype(dtype) == np.longdouble else np.partition(v, rank)[rank]


def ref_filter(M, thr):
    """:496-597"""
    return [{c: v for c, v in r.items() if abs(v) >= thr or c == i} for i, r in enumerate(M)]


def ref_residual(A, LU, dt, rng=None):
    """:602-668: over A's pattern"""
    terms = []
    for i, r in enumerate(A):
        for c, a in r.items():
            d = dt(a) - LU[i].get(c, dt(0))
            terms.append(d * d)
    ss = _sum(terms, dt(0), rng)
    return math.sqrt(ss) if isinstance(ss, float) else np.sqrt(ss)


class Result:
    pass


def ref_par_ilut(A, dtype=np.float64, max_iter=20, delta=1e-2, fill=0.75, rng=None):
    """ilut_numeric (:724-876)"""
    dt = scalar(dtype)
    n = len(A)
    L, U = ref_initial(A, dt)
    res = Result()
    res.nnzL, res.nnzU = sum(len(r) for r in L), sum(len(r) for r in U)
    lim_L, lim_U = int(fill * res.nnzL), int(fill * res.nnzU)
    big = dt(np.finfo(dtype).max)
    prev = cur = big
    it, LU = 0, None
    res.l_threshold = res.u_threshold = 0.0
    while it < max_iter and n > 0:
        if it == 0 or delta <= 0:
            LU = ref_product(L, U, dt, rng)
        Ln, Un = ref_add_candidates(A, L, U, LU, dt)
        ref_sweep(A, Ln, Un, ref_transpose(Un), dt, rng)
        nl, nu = sum(len(r) for r in Ln), sum(len(r) for r in Un)
        tl = ref_select(Ln, max(0, nl - lim_L - 1), dtype)
        tu = ref_select(Un, max(0, nu - lim_U - 1), dtype)
        res.l_threshold, res.u_threshold = float(tl), float(tu)
        L, U = ref_filter(Ln, tl), ref_filter(Un, tu)
        ref_sweep(A, L, U, ref_transpose(U), dt, rng)
        if delta > 0:
            LU = ref_product(L, U, dt, rng)
            cur = ref_residual(A, LU, dt, rng)
            if abs(prev - cur) <= dt(delta):
                it += 1
                break
            prev = cur
        else:
            cur = prev = dt(0)
        it += 1
    res.L, res.U, res.num_iters = [_sorted(r) for r in L], [_sorted(r) for r in U], it
    res.end_rel_res = 0.0 if n == 0 else float(cur)
    return res


# ---------------------------------------------------------------- matrices
def fixture():
    with open(os.path.join(HERE, "golden", "par_ilut_reference_fixture.json")) as f:
        return json.load(f)


def dense_rows(D):
    return [{c: float(v) for c, v in enumerate(r) if v != 0} for r in D]


def diagonal(n):
    return [{i: float(2 + i)} for i in range(n)]


def tridiagonal(n):
    return [_sorted({c: (4.0 if c == i else -1.0 - 0.01 * c) for c in (i - 1, i, i + 1) if 0 <= c < n}) for i in range(n)]


def lattice7(m):
    rows = []
    for z in range(m):
        for y in range(m):
            for x in range(m):
                i = (z * m + y) * m + x
                r = {i: 6.5}
                for d, ok in ((1, x + 1 < m), (-1, x > 0), (m, y + 1 < m), (-m, y > 0), (m * m, z + 1 < m), (-m * m, z > 0)):
                    if ok:
                        r[i + d] = -1.0 + 0.001 * ((i * 7 + d) % 13)
                rows.append(_sorted(r))
    return rows


def banded(n, seed):
    """recipe d: five off-diagonals drawn within +-8 of the row, the diagonal 1 to 2 times 1 + sum |off-diagonals|"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        cols = set(rng.integers(max(0, i - 8), min(n, i + 9), 5).tolist()) - {i}
        r = {int(c): float(rng.uniform(-1, 1)) for c in cols}
        r[i] = float((1 + sum(abs(v) for v in r.values())) * rng.uniform(1, 2))
        rows.append(_sorted(r))
    return rows


def arrow(n, seed=0):
    """the last row and the last column are full: a row longer than one 64-lane pass whose L chain is long"""
    rng = np.random.default_rng(seed)
    rows = [{i: float(rng.uniform(4, 6)), n - 1: float(rng.uniform(-1, 1))} for i in range(n - 1)]
    last = {c: float(rng.uniform(-1, 1)) for c in range(n - 1)}
    last[n - 1] = float(n)
    rows.append(last)
    return rows


def missing_diagonal(n, seed, row):
    """row `row` stores no diagonal and nothing left of it, and no other row stores column `row`: U(row, row) starts as 1, the first sweep
    makes it 0 - 0, and nothing is ever divided by it"""
    rows = banded(n, seed)
    for i, r in enumerate(rows):
        if i == row:
            rows[i] = {c: v for c, v in r.items() if c > row}
        else:
            r.pop(row, None)
    assert rows[row]
    return rows


def zero_u_diagonal():
    """A(0, 0) is stored as 0: U(0, 0) stays 0, so the sweeps meet u_diag == 0 in column 0 and leave L(i, 0) as it was.  Column 0 gets no
    new candidate (there is no k < 0), and with fill_in_limit 3 nothing is dropped, so nothing is ever divided by it."""
    rows = dense_rows([[0, 2, 0, 1, 0], [1, 4, 1, 0, 0], [0.5, 1, 5, 0, 1], [0, 0, 1, 6, 1], [0.25, 0, 0, 1, 7]])
    rows[0] = _sorted({0: 0.0, **rows[0]})
    return rows


class Case:
    def __init__(self, name, rows, **params):
        self.name, self.rows = name, rows
        self.params = dict(max_iter=20, delta=1e-2, fill=0.75)
        self.params.update(params)

    def __repr__(self):
        return self.name

    @property
    def csr(self):
        return Csr.from_rows(self.rows)


@functools.lru_cache(maxsize=None)
def loop_cases(small):
    """small: emulator size.  Otherwise the GPU sizes: recipe d up to n = 2000"""
    fx = fixture()
    out = [Case("fixture", dense_rows(fx["A"])), Case("a-n0", []), Case("a-n1", [{0: 3.0}]), Case("a-diagonal", diagonal(5)),
           Case("b-tridiagonal", tridiagonal(40)), Case("c-lattice7-6", lattice7(6), max_iter=3),
           Case("d-n60-s0", banded(60, 0)), Case("d-n60-s3", banded(60, 3)), Case("d-n300-s1" if small else "d-n2000-s1", banded(300 if small else 2000, 1)),
           Case("e-arrow131", arrow(131)), Case("f-missing-diagonal", missing_diagonal(60, 2, 17)), Case("g-zero-u-diagonal", zero_u_diagonal(), fill=3.0),
           Case("h-fill0.1", banded(60, 4), fill=0.1), Case("h-fill3.0", banded(60, 4), fill=3.0),
           Case("i-no-residual", banded(60, 5), delta=0.0, max_iter=5)]
    if not small:                                               # a row of L * U of more than 256 entries: beyond what one wave of the SpGEMM accumulates
        out.append(Case("e-arrow300", arrow(300, 1)))
    return tuple(out)


def _patterns(res):
    return [tuple(r) for r in res.L], [tuple(r) for r in res.U]


def _deviation(a, b):
    """largest |difference| of the factor values and of end_rel_res between two runs of one pattern"""
    dv = 0.0
    for Ma, Mb in ((a.L, b.L), (a.U, b.U)):
        for ra, rb in zip(Ma, Mb):
            for c in ra:
                x, y = np.longdouble(ra[c]), np.longdouble(rb[c])
                if not (np.isfinite(x) and np.isfinite(y)):
                    assert str(x) == str(y)
                    continue
                dv = max(dv, float(abs(x - y)))
    return dv, abs(a.end_rel_res - b.end_rel_res)


_ANALYSED = {}


def analysed(case):
    """{dtype: (plain run, value tolerance, end_rel_res tolerance)} after asserting the condition of the module docstring"""
    if case.name in _ANALYSED:
        return _ANALYSED[case.name]
    p = case.params
    run = lambda dtype, rng=None: ref_par_ilut(case.rows, dtype, p["max_iter"], p["delta"], p["fill"], rng)
    ld = run(np.longdouble)
    out = {}
    for dtype in (np.float64, np.float32):
        base = run(dtype)
        assert _patterns(base) == _patterns(ld) and base.num_iters == ld.num_iters, "%s: %s and longdouble disagree" % (case.name, np.dtype(dtype).name)
        dv, dr = _deviation(base, ld)
        for k in range(REORDERS):
            other = run(dtype, np.random.default_rng(1000 + k))
            assert _patterns(other) == _patterns(base) and other.num_iters == base.num_iters, "%s: term order %d changes the pattern" % (case.name, k)
            v, r = _deviation(base, other)
            dv, dr = max(dv, v), max(dr, r)
        print("par_ilut case %-22s %-8s iters %d nnzL %d nnzU %d spread: values %.3g end_rel_res %.3g" % (
            case.name, np.dtype(dtype).name, base.num_iters, sum(len(r) for r in base.L), sum(len(r) for r in base.U), dv, dr))
        out[dtype] = (base, MARGIN * dv, MARGIN * dr)
    _ANALYSED[case.name] = out
    return out


# ---------------------------------------------------------------- exact step inputs
def _int_matrix(kind, seed=7):
    rng = np.random.default_rng(seed)
    pow2 = (1.0, 2.0, -1.0, -2.0, 4.0)
    if kind == "arrow":
        n = 131
        rows = [{i: pow2[i % 4], n - 1: float(rng.integers(1, 4))} for i in range(n - 1)]
        last = {c: float(rng.integers(1, 4) * (1 if c % 3 else -1)) for c in range(n - 1)}
        last[n - 1] = 2.0
        return rows + [last]
    n = 70
    rows = []
    for i in range(n):
        cols = set(rng.integers(max(0, i - 3), min(n, i + 4), 4).tolist()) - {i}
        r = {int(c): float(rng.integers(1, 4) * rng.choice((-1, 1))) for c in cols}
        r[i] = pow2[int(rng.integers(0, 5))]
        rows.append(_sorted(r))
    return rows


@functools.lru_cache(maxsize=None)
def exact_inputs(kind):
    """A, the old L and U (some entries of the initial factors dropped), LU = L * U, the candidates, the sweep's result, a filter and the
    residual, every one the same bits in float32, float64 and longdouble and under a random term order (asserted here)"""
    A = _int_matrix(kind)
    rng0 = np.random.default_rng(11)

    def build(dtype, rng):
        dt = scalar(dtype)
        L, U = ref_initial(A, dt)
        drop = np.random.default_rng(5)
        for i in range(len(A)):
            for M in (L, U):
                for c in list(M[i]):
                    if c != i and drop.random() < 0.3:
                        del M[i][c]
        LU = ref_product(L, U, dt, rng)
        Ln, Un = ref_add_candidates(A, L, U, LU, dt)
        Ut = ref_transpose(Un)
        Ls, Us = [dict(r) for r in Ln], [dict(r) for r in Un]
        ref_sweep(A, Ls, Us, Ut, dt, rng)
        thr = dt(2)
        Lf = ref_filter(Ls, thr)
        resid = ref_residual(A, LU, dt, rng)
        return dict(A=A, L=L, U=U, LU=LU, Ln=Ln, Un=Un, Ut=Ut, Ls=Ls, Us=Us, thr=2.0, Lf=Lf, resid=float(resid))

    base = build(np.float64, None)
    as64 = lambda M: [(c, float(v)) for r in M for c, v in r.items()]
    for dtype, rng in ((np.float32, None), (np.longdouble, None), (np.float64, rng0), (np.float32, rng0)):
        other = build(dtype, rng)
        for key in ("LU", "Ln", "Un", "Ls", "Us", "Lf"):
            assert as64(other[key]) == as64(base[key]), "exact_inputs(%s): %s is not exact in %s" % (kind, key, np.dtype(dtype).name)
        assert other["resid"] == float(np.dtype(dtype).type(base["resid"])), (kind, other["resid"], base["resid"])
    assert all(math.isfinite(v) for _, v in as64(base["Ls"]) + as64(base["Us"]))
    return base


def select_values(count, seed):
    """arbitrary magnitudes with ties, zeros, -0.0, denormals and Inf"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(count) * 10.0 ** rng.integers(-3, 4, count)
    v[rng.integers(0, count, count // 4)] = np.round(v[rng.integers(0, count, count // 4)], 0)     # ties
    v[rng.integers(0, count, count // 8)] = 1.5
    v[rng.integers(0, count, count // 8)] = -1.5
    v[:10] = [0.0, -0.0, 5e-324, -1e-310, np.inf, -np.inf, 1e-45, -1e-40, 3e-39, 1e-40]     # float64 and float32 denormals (with a tie)
    return v


# ---------------------------------------------------------------- running the library
def _up(be, csr, od, vd):
    return (be.from_numpy(csr.row_map.astype(od)), be.from_numpy(csr.entries.astype(np.int32)), be.from_numpy(np.asarray(csr.values).astype(vd)))


def _ptrs(be, t):
    return tuple(be.ptr(a) for a in t)


def _down(be, n, rm, ent, val):
    rm = be.to_numpy(rm).astype(np.int64)
    nnz = int(rm[-1])
    return Csr(n, rm, be.to_numpy(ent)[:nnz], be.to_numpy(val)[:nnz])


def same_csr(got, rows, dtype, tol=0.0):
    """the pattern exactly, the values within tol (0: the same bits)"""
    exp = Csr.from_rows(rows, dtype)
    assert np.array_equal(got.row_map, exp.row_map), "row maps differ"
    assert np.array_equal(got.entries, exp.entries), "patterns differ"
    g, e = np.asarray(got.values), np.asarray(exp.values)
    assert g.dtype == e.dtype
    if tol == 0.0:
        assert np.array_equal(g, e) and np.array_equal(np.signbit(g), np.signbit(e)), "values differ: max %g" % (np.abs(g - e).max() if g.size else 0)
    else:
        fin = np.isfinite(e)
        assert np.array_equal(fin, np.isfinite(g))
        err = float(np.abs(g[fin].astype(np.float64) - e[fin].astype(np.float64)).max()) if fin.any() else 0.0
        assert err <= tol, "values differ by %g > %g" % (err, tol)


class Factored:
    """one kkamd_par_ilut handle on one case through the Python front end"""

    def __init__(self, kk, be, case, offset_dtype=np.int32, lanes=0):
        self.kk, self.be, self.case, self.od = kk, be, case, offset_dtype
        p = case.params
        self.kh = kk.KokkosKernelsHandle(be)
        self.kh.create_par_ilut_handle(p["max_iter"], p["delta"], p["fill"])
        self.ih = self.kh.get_par_ilut_handle()
        if lanes:
            self.ih.set("lanes_per_row", lanes)
        self.A = case.csr
        self.n = self.A.n
        self.A_rm, self.A_ent = be.from_numpy(self.A.row_map.astype(offset_dtype)), be.from_numpy(self.A.entries)
        self.L_rm, self.U_rm = be.from_numpy(np.full(self.n + 1, -1, dtype=offset_dtype)), be.from_numpy(np.full(self.n + 1, -1, dtype=offset_dtype))
        kk.par_ilut_symbolic(self.kh, self.A_rm, self.A_ent, self.L_rm, self.U_rm)

    def numeric(self, dtype, values=None):
        be = self.be
        val = be.from_numpy(np.asarray(self.A.values if values is None else values).astype(dtype))
        L_ent, L_val, U_ent, U_val = self.kk.par_ilut_numeric(self.kh, self.A_rm, self.A_ent, val, self.L_rm, self.U_rm)
        return _down(be, self.n, self.L_rm, L_ent, L_val), _down(be, self.n, self.U_rm, U_ent, U_val)

    def close(self):
        self.kh.destroy_par_ilut_handle()


def check_loop(kk, be, case, offset_dtype, dtype, lanes=0):
    base, tol, tol_res = analysed(case)[dtype]
    f = Factored(kk, be, case, offset_dtype, lanes)
    assert (f.ih.get_nnzL(), f.ih.get_nnzU(), f.ih.get_nrows()) == (base.nnzL, base.nnzU, len(case.rows))
    L, U = f.numeric(dtype)
    same_csr(L, base.L, dtype, tol if tol > 0 else 0.0)
    same_csr(U, base.U, dtype, tol if tol > 0 else 0.0)
    assert f.ih.get_num_iters() == base.num_iters
    assert abs(f.ih.get_end_rel_res() - base.end_rel_res) <= tol_res, (f.ih.get_end_rel_res(), base.end_rel_res, tol_res)
    if base.num_iters > 0:
        assert abs(f.ih.get_real("l_threshold") - base.l_threshold) <= max(tol, 0.0) and abs(f.ih.get_real("u_threshold") - base.u_threshold) <= max(tol, 0.0)
    assert (f.ih.get("nnzL_out"), f.ih.get("nnzU_out")) == (L.nnz, U.nnz)
    f.close()
    return L, U


def _step_handle(kk, be, lanes):
    kh = kk.KokkosKernelsHandle(be)
    kh.create_par_ilut_handle()
    ih = kh.get_par_ilut_handle()
    ih.set("lanes_per_row", lanes)
    return kh, ih


def check_steps(kk, be, kind, offset_dtype, dtype, lanes):
    """add_candidates, one sweep, the filter and the residual on exact inputs: the same bits as the restated steps"""
    cap, lib = kk._capi, be.lib
    x = exact_inputs(kind)
    n = len(x["A"])
    ot, vt = (cap.I64 if np.dtype(offset_dtype) == np.int64 else cap.I32), (cap.F64 if np.dtype(dtype) == np.float64 else cap.F32)
    kh, ih = _step_handle(kk, be, lanes)
    dev = {k: _up(be, Csr.from_rows(x[k]), offset_dtype, dtype) for k in ("A", "L", "U", "LU", "Ln", "Un", "Ut", "Ls")}
    st = be.stream()
    # add_candidates: the sizing call, then the fill
    Ln_rm, Un_rm = be.from_numpy(np.full(n + 1, -1, dtype=offset_dtype)), be.from_numpy(np.full(n + 1, -1, dtype=offset_dtype))
    nl, nu = C.c_int64(), C.c_int64()
    head = (ih.h, n) + _ptrs(be, dev["A"]) + _ptrs(be, dev["L"]) + _ptrs(be, dev["U"]) + _ptrs(be, dev["LU"]) + (Csr.from_rows(x["LU"]).nnz,)
    cap.check(lib, lib.kkamd_par_ilut_add_candidates(*head, be.ptr(Ln_rm), None, None, 0, be.ptr(Un_rm), None, None, 0, C.byref(nl), C.byref(nu), ot, vt, st))
    exp_Ln, exp_Un = Csr.from_rows(x["Ln"], dtype), Csr.from_rows(x["Un"], dtype)
    assert (nl.value, nu.value) == (exp_Ln.nnz, exp_Un.nnz)
    Ln_ent, Ln_val = be.from_numpy(np.full(nl.value, -1, dtype=np.int32)), be.from_numpy(np.zeros(nl.value, dtype=dtype))
    Un_ent, Un_val = be.from_numpy(np.full(nu.value, -1, dtype=np.int32)), be.from_numpy(np.zeros(nu.value, dtype=dtype))
    assert lib.kkamd_par_ilut_add_candidates(*head, be.ptr(Ln_rm), be.ptr(Ln_ent), be.ptr(Ln_val), nl.value - 1, be.ptr(Un_rm), be.ptr(Un_ent), be.ptr(Un_val),
                                             nu.value, C.byref(nl), C.byref(nu), ot, vt, st) == cap.ERR_INVALID_ARG
    assert (be.to_numpy(Ln_ent) == -1).all()
    cap.check(lib, lib.kkamd_par_ilut_add_candidates(*head, be.ptr(Ln_rm), be.ptr(Ln_ent), be.ptr(Ln_val), nl.value, be.ptr(Un_rm), be.ptr(Un_ent), be.ptr(Un_val),
                                                     nu.value, C.byref(nl), C.byref(nu), ot, vt, st))
    same_csr(_down(be, n, Ln_rm, Ln_ent, Ln_val), x["Ln"], dtype)
    same_csr(_down(be, n, Un_rm, Un_ent, Un_val), x["Un"], dtype)
    # one sweep, in place, on the candidates
    Lw, Uw = dev["Ln"], dev["Un"]
    cap.check(lib, lib.kkamd_par_ilut_sweep(ih.h, n, *_ptrs(be, dev["A"]), *_ptrs(be, Lw), *_ptrs(be, Uw), *_ptrs(be, dev["Ut"]), ot, vt, st))
    same_csr(_down(be, n, *Lw), x["Ls"], dtype)
    same_csr(_down(be, n, *Uw), x["Us"], dtype)
    # the filter of the swept L at threshold 2
    thr = be.from_numpy(np.array([x["thr"]], dtype=dtype))
    O_rm = be.from_numpy(np.full(n + 1, -1, dtype=offset_dtype))
    cnt = C.c_int64()
    fhead = (ih.h, n) + _ptrs(be, dev["Ls"]) + (be.ptr(thr), be.ptr(O_rm))
    cap.check(lib, lib.kkamd_par_ilut_filter(*fhead, None, None, 0, C.byref(cnt), ot, vt, st))
    exp_f = Csr.from_rows(x["Lf"], dtype)
    assert cnt.value == exp_f.nnz and exp_f.nnz < Csr.from_rows(x["Ls"]).nnz
    O_ent, O_val = be.from_numpy(np.full(cnt.value, -1, dtype=np.int32)), be.from_numpy(np.zeros(cnt.value, dtype=dtype))
    assert lib.kkamd_par_ilut_filter(*fhead, be.ptr(O_ent), be.ptr(O_val), cnt.value - 1, C.byref(cnt), ot, vt, st) == cap.ERR_INVALID_ARG
    cap.check(lib, lib.kkamd_par_ilut_filter(*fhead, be.ptr(O_ent), be.ptr(O_val), cnt.value, C.byref(cnt), ot, vt, st))
    same_csr(_down(be, n, O_rm, O_ent, O_val), x["Lf"], dtype)
    # the residual: a sum of squares of integers and a correctly rounded square root
    r = C.c_double()
    cap.check(lib, lib.kkamd_par_ilut_residual(ih.h, n, *_ptrs(be, dev["A"]), *_ptrs(be, dev["LU"]), C.byref(r), ot, vt, st))
    assert r.value == float(np.dtype(dtype).type(x["resid"])) and r.value > 0
    kh.destroy_par_ilut_handle()


def check_select(kk, be, count, dtype, lanes=0):
    cap, lib = kk._capi, be.lib
    kh, ih = _step_handle(kk, be, lanes)
    v = select_values(count, count).astype(dtype)
    mag = np.abs(v)
    d_v, d_t = be.from_numpy(v), be.from_numpy(np.zeros(1, dtype=dtype))
    vt = cap.F64 if np.dtype(dtype) == np.float64 else cap.F32
    order = np.sort(mag)
    tie = int(np.searchsorted(order, 1.5)) + 1                 # inside the run of 1.5s
    for rank in (0, 1, 2, 5, count // 2, tie, count - 3, count - 1):
        cap.check(lib, lib.kkamd_par_ilut_select(ih.h, count, be.ptr(d_v), rank, be.ptr(d_t), vt, be.stream()))
        got = be.to_numpy(d_t)[0]
        exp = np.partition(mag, rank)[rank]
        assert got == exp and got.dtype == exp.dtype, (rank, got, exp)
    assert order[tie] == 1.5 and order[0] == 0 and np.isinf(order[-1])
    for bad in (-1, count):
        assert lib.kkamd_par_ilut_select(ih.h, count, be.ptr(d_v), bad, be.ptr(d_t), vt, be.stream()) == cap.ERR_INVALID_ARG
    kh.destroy_par_ilut_handle()


def _status(kk, fn):
    try:
        fn()
    except kk.KkamdError as e:
        return e.status, str(e)
    raise AssertionError("no error raised")


def check_statuses(kk, be):
    cap, lib = kk._capi, be.lib
    i32 = lambda a: be.from_numpy(np.array(a, dtype=np.int32))
    kh = kk.KokkosKernelsHandle(be)
    try:
        kk.par_ilut_symbolic(kh, i32([0, 1]), i32([0]), i32([0, 0]), i32([0, 0]))
        raise AssertionError("no PAR_ILUT handle, no error")
    except ValueError:
        pass
    kh.create_par_ilut_handle()
    ih = kh.get_par_ilut_handle()
    assert (ih.get_max_iter(), ih.get_residual_norm_delta_stop(), ih.get_fill_in_limit(), ih.get_async_update(), ih.get_verbose()) == (20, 1e-2, 0.75, False, False)
    assert ih.get_num_iters() == -1 and ih.get_end_rel_res() == -1 and not ih.is_symbolic_complete() and ih.get("lanes_per_row") == 0
    out = lambda: (i32(np.full(4, -1)), i32(np.full(4, -1)))
    # structural faults name the smallest offending row (row 1 and row 2 are faulty in every case)
    for row_map, entries, word in (((0, 1, 4, 7), [0, 0, 1, 0, 2, 2, 1], "sorted"), ((0, 1, 3, 5), [0, 1, 3, 2, -1], "outside"),
                                   ((0, 2, 1, 3), [0, 1, 1], "not ascending"), ((0, 1, 3, 5), [0, 1, 1, 0, 2], "sorted")):
        L_rm, U_rm = out()
        st, msg = _status(kk, lambda: kk.par_ilut_symbolic(kh, i32(row_map), i32(entries), L_rm, U_rm))
        assert st == cap.ERR_INVALID_ARG and "row 1:" in msg and word in msg, msg
        assert not ih.is_symbolic_complete() and (be.to_numpy(L_rm) == -1).all()
    # numeric before symbolic, copy_factors before numeric
    case = loop_cases(True)[0]
    A = case.csr
    A_rm, A_ent, A_val = i32(A.row_map), i32(A.entries), be.from_numpy(A.values)
    L_rm, U_rm = i32(np.zeros(5)), i32(np.zeros(5))
    try:
        kk.par_ilut_numeric(kh, A_rm, A_ent, A_val, L_rm, U_rm)
        raise AssertionError("numeric before symbolic")
    except ValueError as e:
        assert "symbolic" in str(e)
    assert lib.kkamd_par_ilut_copy_factors(ih.h, None, None, 0, None, None, 0, be.stream()) == cap.ERR_STATE
    kk.par_ilut_symbolic(kh, A_rm, A_ent, L_rm, U_rm)
    assert ih.is_symbolic_complete() and (ih.get_nnzL(), ih.get_nnzU()) == (10, 8)
    assert lib.kkamd_par_ilut_copy_factors(ih.h, None, None, 0, None, None, 0, be.stream()) == cap.ERR_STATE
    args = (ih.h, 4, be.ptr(A_rm), be.ptr(A_ent), be.ptr(A_val), be.ptr(L_rm), be.ptr(U_rm))
    assert lib.kkamd_par_ilut_numeric(*args, cap.I32, 5, be.stream()) == cap.ERR_UNSUPPORTED
    assert lib.kkamd_par_ilut_numeric(ih.h, 5, *args[2:], cap.I32, cap.F64, be.stream()) == cap.ERR_INVALID_ARG
    assert lib.kkamd_par_ilut_numeric(*args, cap.I64, cap.F64, be.stream()) == cap.ERR_INVALID_ARG
    # a short capacity carries the true count and writes nothing
    L_ent, L_val, U_ent, U_val = kk.par_ilut_numeric(kh, A_rm, A_ent, A_val, L_rm, U_rm)
    nl, nu = ih.get("nnzL_out"), ih.get("nnzU_out")
    for dl, du, which, need in ((1, 0, "L", nl), (0, 1, "U", nu)):
        e1, v1, e2, v2 = i32(np.full(nl, -1)), be.from_numpy(np.zeros(nl)), i32(np.full(nu, -1)), be.from_numpy(np.zeros(nu))
        rc = lib.kkamd_par_ilut_copy_factors(ih.h, be.ptr(e1), be.ptr(v1), nl - dl, be.ptr(e2), be.ptr(v2), nu - du, be.stream())
        assert rc == cap.ERR_INVALID_ARG and ("%s_entries" % which) in lib.kkamd_last_error().decode() and ("at least %d" % need) in lib.kkamd_last_error().decode()
        assert (be.to_numpy(e1) == -1).all() and (be.to_numpy(e2) == -1).all()
    # knobs out of range, unknown keys
    for key, bad in (("lanes_per_row", 3), ("lanes_per_row", 128), ("lanes_per_row", -1), ("max_iter", -1), ("max_iter", 1.5), ("fill_in_limit", -0.5),
                     ("async_update", 2), ("verbose", 7), ("residual_norm_delta_stop", float("nan")), ("nonsense", 1)):
        st, msg = _status(kk, lambda: ih.set(key, bad))
        assert st == cap.ERR_INVALID_ARG, (key, bad)
    assert _status(kk, lambda: ih.get("nonsense"))[0] == cap.ERR_INVALID_ARG and _status(kk, lambda: ih.get_real("nonsense"))[0] == cap.ERR_INVALID_ARG
    ih.set_async_update(True)                                  # recorded, without effect
    assert ih.get_async_update()
    h = C.c_void_p()
    assert lib.kkamd_par_ilut_create(C.byref(h), -1, 1e-2, 0.75, 0, 0) == cap.ERR_INVALID_ARG
    assert lib.kkamd_par_ilut_create(C.byref(h), 20, 1e-2, -1.0, 0, 0) == cap.ERR_INVALID_ARG
    kh.destroy_par_ilut_handle()
    assert kh.get_par_ilut_handle() is None


def check_fixture(kk, be):
    """the reference's own test: nnzL 10, nnzU 8 and the expected factors to 2 decimals (Test_Sparse_par_ilut.hpp:97-98,160-170)"""
    fx = fixture()
    for dtype in (np.float64, np.float32):
        f = Factored(kk, be, loop_cases(True)[0])
        assert (f.ih.get_nnzL(), f.ih.get_nnzU()) == (fx["nnzL"], fx["nnzU"])
        L, U = f.numeric(dtype)
        for M, exp in ((L, fx["L"]), (U, fx["U"])):
            dense = np.zeros((4, 4))
            for i in range(4):
                for p in range(M.row_map[i], M.row_map[i + 1]):
                    dense[i, M.entries[p]] = M.values[p]
            assert np.array_equal(np.round(dense, 2) + 0.0, np.array(exp)), (dense, exp)
        assert f.ih.get_num_iters() == 4
        f.close()


PRECOND_N, PRECOND_SEED, PRECOND_M, PRECOND_TOL = 300, 6, 15, 1e-8


@functools.lru_cache(maxsize=None)
def precond_case():
    """par_ilut, then LUPrec, then gmres (Test_Sparse_par_ilut.hpp:177-300) on a recipe-d matrix: the restated loops on the CPU take at least
    2 iterations fewer with the preconditioner than without"""
    import gmres_cases as gc
    case = Case("precond", banded(PRECOND_N, PRECOND_SEED))
    n = PRECOND_N
    dense = lambda rows: np.array([[r.get(c, 0.0) for c in range(n)] for r in rows])
    D = dense(case.rows)
    f = ref_par_ilut(case.rows)
    Ld, Ud = dense(f.L), dense(f.U)
    M = lambda v: np.linalg.solve(Ud, np.linalg.solve(Ld, v))
    b, x0 = np.ones(n), np.zeros(n)
    plain = gc.restated_gmres(D, b, x0, PRECOND_M, PRECOND_TOL, 50, "CGS2", np.float64)
    pre = gc.restated_gmres(D, b, x0, PRECOND_M, PRECOND_TOL, 50, "CGS2", np.float64, M)
    assert plain.flag == "Conv" and pre.flag == "Conv" and pre.num_iters + 2 <= plain.num_iters, (plain.num_iters, pre.num_iters)
    return case, D, plain.num_iters, pre.num_iters


def check_precond(kk, be):
    case, D, it_plain, it_pre = precond_case()
    n = PRECOND_N
    f = Factored(kk, be, case)
    val = be.from_numpy(np.asarray(f.A.values))
    L_ent, L_val, U_ent, U_val = kk.par_ilut_numeric(f.kh, f.A_rm, f.A_ent, val, f.L_rm, f.U_rm)
    A = kk.CrsMatrix(n, n, f.A_rm, f.A_ent, val, backend=be)
    L, U = kk.CrsMatrix(n, n, f.L_rm, L_ent, L_val, backend=be), kk.CrsMatrix(n, n, f.U_rm, U_ent, U_val, backend=be)
    kh = kk.KokkosKernelsHandle(be)
    kh.create_gmres_handle(PRECOND_M, PRECOND_TOL)
    gh = kh.get_gmres_handle()
    iters = []
    for P in (None, kk.LUPrec(L, U)):
        gh.reset_handle(PRECOND_M, PRECOND_TOL)
        B, X = be.from_numpy(np.ones(n)), be.from_numpy(np.zeros(n))
        kk.gmres(kh, A, B, X, P)
        x = be.to_numpy(X)
        end = float(np.linalg.norm(np.ones(n) - D @ x) / np.sqrt(n))
        print("par_ilut precond: %s iterations %d true relative residual %.3g" % ("plain" if P is None else "LUPrec", gh.get_num_iters(), end))
        assert gh.get_conv_flag_val() == "Conv" and end < PRECOND_TOL and gh.get_num_iters() > 0
        iters.append(gh.get_num_iters())
        if P is not None:
            P.destroy()
    assert iters[1] < iters[0], iters
    kh.destroy_gmres_handle()
    f.close()


def check_repeated_numeric(kk, be, dtype=np.float64):
    """new values on one handle: each call equals a fresh handle's result, bit for bit"""
    case = loop_cases(True)[6]
    f = Factored(kk, be, case)
    first = f.numeric(dtype)
    scaled = np.asarray(case.csr.values) * 2.0
    second = f.numeric(dtype, scaled)
    again = f.numeric(dtype)
    g = Factored(kk, be, Case("scaled", Csr(case.csr.n, case.csr.row_map, case.csr.entries, scaled).rows()))
    fresh = g.numeric(dtype)
    for a, b in ((first, again), (second, fresh)):
        for Ma, Mb in zip(a, b):
            assert np.array_equal(Ma.row_map, Mb.row_map) and np.array_equal(Ma.entries, Mb.entries) and np.array_equal(Ma.values, Mb.values)
    assert not np.array_equal(first[1].values, second[1].values)
    assert f.ih.get("host_syncs") > 0 and f.ih.get("launches") > 0 and f.ih.get("plan_bytes") > 0
    f.close(); g.close()
