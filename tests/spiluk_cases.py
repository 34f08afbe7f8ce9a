"""Generated inputs of the ILU(k) tests (CPU only; shared by test_emu_spiluk.py and test_gpu_spiluk.py).

Patterns of A (numpy.random.default_rng with fixed seeds; `small` cuts them to emulator size, n <= 300), each with the entries of
every row sorted by column and shuffled, the diagonal stored:
  a   diagonal only: one level as wide as the matrix (the reference's dense work array is level_maxrows x nrows)
  b   random, 0-3 off-diagonal entries per row anywhere in the row: few wide levels and a narrow tail
  c   long rows, up to 150 (small) / 300 off-diagonal entries: beyond one pass of 64 lanes and beyond the LDS staging cap
  d   tridiagonal: one row per level, all chained
  e27, e7  the 27-point and the 7-point lattice
  f0, f1   n = 0 and n = 1
g_cases() gives the two special matrices of the 1e6 rule: diagonals missing from A, and a pivot that cancels to exactly zero.

Restatements of the reference:
  reference_symbolic  the sum-rule fill loop of sparse/impl/KokkosSparse_spiluk_symbolic_impl.hpp:282-389 (entries of A have level 0;
                      eliminating row i by pivot j, pivots ascending, gives column c of U row j the level lev(i,j) + lev(j,c) + 1, kept
                      when <= fill_lev; an existing entry takes the minimum), rows sorted as sort_crs_graph leaves them (:395-398);
                      the level sets of L (:400-402) are sptrsv_cases.reference_levels
  reference_numeric   the recurrence of sparse/impl/KokkosSparse_spiluk_numeric_impl.hpp:438-551, one pivot at a time in ascending
                      order, every operation rounded to the value type

Two value classes:
  exact    built backwards from chosen factors: walking the rows in order, a position of A takes a free factor entry (off-diagonal
           integers 1 <= |v| <= 3, U diagonals from {0.5, 1, 2, 4, -1, -2}, but +-1 in every column that holds a fill position of L)
           and a_ic = sum_{k <= min(i,c)} l_ik u_kc; a fill position is forced to -sum_{k < min} l_ik u_kc (divided by u_cc = +-1 in L).
           ILU(k) of this A is exactly (L, U).  Every partial sum is an integer or a half-integer; the generator asserts
           2 max_ic sum |l_ik| |u_kc| < 2^24 (the factor 2 for the half-integers), so fp32 and fp64 both give the factors bit for
           bit whether or not x - f * u is contracted.  Used for every pattern at k = 0 and for b and d at k = 1, 2 (on lattices
           the forced values explode at k = 1).
  rounded  off-diagonals uniform in (-1, 1), diagonal (1 + sum |off|) times uniform(1, 2) with a random sign; checked by
           identity_check.
"""
import functools
import heapq

import numpy as np

import sptrsv_cases as sc

LANES, CHAIN_ROWS, CHAIN_LEVELS = sc.LANES, sc.CHAIN_ROWS, sc.CHAIN_LEVELS
_INF = np.int64(1) << 40


def expected_launches(level_ptr, chain_rows, chain_levels):
    """(launches, chain_launches, chained_levels) of one numeric call: the arithmetic of sptrsv_cases.expected_launches with chaining
    governed by chain_rows alone (SPILUK has one algorithm)"""
    return sc.expected_launches(np.diff(level_ptr), sc.ALGORITHMS["SEQLVLSCHD_TP1CHAIN"], chain_rows, chain_levels)


class Symbolic:
    """graphs of L and U (row maps int64, entries int32) and the level sets of L, as the reference leaves them"""

    def __init__(self, n, L_row_map, L_entries, U_row_map, U_entries):
        self.n, self.L_row_map, self.L_entries, self.U_row_map, self.U_entries = n, L_row_map, L_entries, U_row_map, U_entries
        level, per_level, grouped = sc.reference_levels(n, L_row_map, L_entries, True)
        self.level_list, self.level_idx = level, grouped
        self.level_ptr = np.concatenate([[0], np.cumsum(per_level)]).astype(np.int32)
        self.L_rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(L_row_map))
        self.U_rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(U_row_map))

    @property
    def nnzL(self): return int(self.L_entries.shape[0])

    @property
    def nnzU(self): return int(self.U_entries.shape[0])

    @property
    def num_levels(self): return int(self.level_ptr.shape[0]) - 1

    @property
    def max_level_rows(self): return int(np.diff(self.level_ptr).max()) if self.num_levels else 0


def reference_symbolic(n, row_map, entries, fill_lev):
    lev = np.full(n, _INF, dtype=np.int64)                # level of (i, c) in the row under way
    U_cols, U_levs, L_cols = [], [], []
    for i in range(n):
        c = entries[row_map[i]:row_map[i + 1]].astype(np.int64)
        c = c[c != i]
        lev[c] = 0
        touched = [c]
        heap = c[c < i].tolist()
        heapq.heapify(heap)
        while heap:                                         # pivots in ascending column order, fill-in included
            j = heapq.heappop(heap)
            cols, lev1 = U_cols[j][1:], lev[j] + U_levs[j][1:] + 1
            keep = (lev1 <= fill_lev) & (cols != i)
            cols, lev1 = cols[keep], lev1[keep]
            new = cols[lev[cols] == _INF]
            for x in new[new < i].tolist():
                heapq.heappush(heap, x)
            lev[cols] = np.minimum(lev[cols], lev1)
            touched.append(new)
        t = np.unique(np.concatenate(touched))
        lo, up = t[t < i], t[t > i]
        L_cols.append(np.concatenate([lo, [i]]))
        U_cols.append(np.concatenate([[i], up]).astype(np.int64))
        U_levs.append(np.concatenate([[0], lev[up]]).astype(np.int64))
        lev[t] = _INF

    def crs(rows):
        rm = np.zeros(n + 1, dtype=np.int64)
        if n:
            np.cumsum(np.array([r.shape[0] for r in rows], dtype=np.int64), out=rm[1:])
        return rm, (np.concatenate(rows) if n else np.zeros(0)).astype(np.int32)

    return Symbolic(n, *crs(L_cols), *crs(U_cols))


def reference_numeric(pat_row_map, pat_entries, values, sym, dtype):
    """(L_values, U_values) in `dtype`: one pivot at a time, product and difference rounded separately"""
    n = sym.n
    Lv, Uv = np.zeros(sym.nnzL, dtype=dtype), np.zeros(sym.nnzU, dtype=dtype)
    w = np.zeros(n, dtype=dtype)
    inrow = np.zeros(n, dtype=bool)
    values = values.astype(dtype)
    for i in range(n):
        ls, le, us, ue = sym.L_row_map[i], sym.L_row_map[i + 1], sym.U_row_map[i], sym.U_row_map[i + 1]
        lc, uc = sym.L_entries[ls:le - 1].astype(np.int64), sym.U_entries[us:ue].astype(np.int64)
        inrow[lc] = True; inrow[uc] = True
        w[lc] = 0; w[uc] = 0
        a = slice(pat_row_map[i], pat_row_map[i + 1])
        w[pat_entries[a]] = values[a]
        for k in lc:
            f = w[k] / Uv[sym.U_row_map[k]]
            w[k] = f
            cols = sym.U_entries[sym.U_row_map[k] + 1:sym.U_row_map[k + 1]].astype(np.int64)
            m = inrow[cols]
            prod = (f * Uv[sym.U_row_map[k] + 1:sym.U_row_map[k + 1]][m]).astype(dtype)
            w[cols[m]] = (w[cols[m]] - prod).astype(dtype)
        if w[i] == 0:
            w[i] = 1e6
        Lv[ls:le - 1] = w[lc]; Lv[le - 1] = 1
        Uv[us:ue] = w[uc]
        inrow[lc] = False; inrow[uc] = False
    return Lv, Uv


class Pattern:
    """the graph of one square A (row_map int64, entries int32, diagonal stored)"""

    def __init__(self, name, n, shuffled, row_map, entries, seed):
        self.name, self.n, self.shuffled, self.row_map, self.entries, self._seed = name, n, shuffled, row_map, entries, seed
        self._sym, self._exact = {}, {}

    def __repr__(self):
        return "%s-%s" % (self.name, "shuffled" if self.shuffled else "sorted")

    @functools.cached_property
    def rows(self):
        return np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.row_map))

    def symbolic(self, fill_lev):
        if fill_lev not in self._sym:
            self._sym[fill_lev] = reference_symbolic(self.n, self.row_map, self.entries, fill_lev)
        return self._sym[fill_lev]

    def exact(self, fill_lev):
        """(A_values, L_values, U_values) as float64 arrays holding numbers that fp32 represents too"""
        if fill_lev not in self._exact:
            self._exact[fill_lev] = _exact_values(self, self.symbolic(fill_lev), np.random.default_rng(self._seed + 1 + fill_lev))
        return self._exact[fill_lev]

    @functools.cached_property
    def rounded(self):
        """A_values in float64"""
        rng = np.random.default_rng(self._seed + 7)
        rows, cols, n = self.rows, self.entries.astype(np.int64), self.n
        val = rng.uniform(-1.0, 1.0, cols.shape[0])
        isdiag = rows == cols
        s = np.zeros(n)
        np.add.at(s, rows[~isdiag], np.abs(val[~isdiag]))
        d = (1.0 + s) * rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
        val[isdiag] = d[rows[isdiag]]
        return val


def _exact_values(pat, sym, rng):
    n = pat.n
    Lv, Uv = np.zeros(sym.nnzL), np.zeros(sym.nnzU)
    aL, aU = np.zeros(sym.nnzL), np.zeros(sym.nnzU)           # a_ic at the positions of the pattern (meaningful where A has an entry)
    skeys = np.sort(pat.rows * n + pat.entries)
    inS_L = np.isin(sym.L_rows * n + sym.L_entries, skeys)
    inS_U = np.isin(sym.U_rows * n + sym.U_entries, skeys)
    offL = sym.L_entries != sym.L_rows
    unit_col = np.zeros(n, dtype=bool)                        # columns that hold a fill position of L: u_cc = +-1 there
    unit_col[sym.L_entries[offL & ~inS_L]] = True
    acc, absacc = np.zeros(n), np.zeros(n)
    worst = 0.0
    for i in range(n):
        ls, le, us, ue = sym.L_row_map[i], sym.L_row_map[i + 1], sym.U_row_map[i], sym.U_row_map[i + 1]
        touched = [sym.U_entries[us:ue]]
        drawn = (rng.integers(1, 4, le - ls) * rng.choice([-1, 1], le - ls)).astype(np.float64)
        for p in range(ls, le - 1):
            k = sym.L_entries[p]
            ukk = Uv[sym.U_row_map[k]]
            if inS_L[p]:
                l = drawn[p - ls]
                aL[p] = acc[k] + l * ukk
            else:
                l = -acc[k] / ukk
            Lv[p] = l
            worst = max(worst, absacc[k] + abs(l * ukk))
            r = slice(sym.U_row_map[k] + 1, sym.U_row_map[k + 1])
            cols = sym.U_entries[r]
            acc[cols] += l * Uv[r]
            absacc[cols] += np.abs(l * Uv[r])
            touched.append(cols)
        Lv[le - 1] = 1.0
        uc = sym.U_entries[us:ue]
        free = inS_U[us:ue].copy()
        assert free[0], "%r: the exact class needs the diagonal in A" % pat
        draw = (rng.integers(1, 4, ue - us) * rng.choice([-1, 1], ue - us)).astype(np.float64)
        draw[0] = rng.choice([1.0, -1.0]) if unit_col[i] else rng.choice([0.5, 1.0, 2.0, 4.0, -1.0, -2.0])
        Uv[us:ue] = np.where(free, draw, -acc[uc])
        aU[us:ue] = np.where(free, acc[uc] + draw, 0.0)
        if ue > us:
            worst = max(worst, float((absacc[uc] + np.abs(Uv[us:ue])).max()))
        for t in touched:
            acc[t] = 0.0; absacc[t] = 0.0
    assert 2 * worst < 2 ** 24, "%r: partial sums are not exact in fp32 (bound %g)" % (pat, worst)
    pkeys = np.concatenate([(sym.L_rows * n + sym.L_entries)[offL], sym.U_rows * n + sym.U_entries])
    pvals = np.concatenate([aL[offL], aU])
    order = np.argsort(pkeys)
    A = pvals[order][np.searchsorted(pkeys[order], pat.rows * n + pat.entries)] if n else np.zeros(0)
    return A, Lv, Uv


def identity_check(pat, sym, A_values, L_values, U_values, dtype):
    """The ILU identity (L U)_P = A_P: for every position (i,c) of the pattern P of L and U, evaluated in the next wider format,
    |a_ic - sum_{k <= min(i,c), in P} l_ik u_kc| <= 2 (m + 2) u sum |l_ik| |u_kc|, m the number of terms, a_ic = 0 where A stores
    nothing, u = 2^-53 or 2^-24: the substitution bound of sptrsv_cases.residual_check, each factor entry being the result of one
    substitution of m terms.  The arrays are what the factorisation saw and gave, in `dtype`.  Returns the largest ratio."""
    wide, u = (np.longdouble, 2.0 ** -53) if np.dtype(dtype) == np.dtype(np.float64) else (np.float64, 2.0 ** -24)
    assert A_values.dtype == np.dtype(dtype) and L_values.dtype == np.dtype(dtype) and U_values.dtype == np.dtype(dtype)
    assert np.isfinite(L_values).all() and np.isfinite(U_values).all()
    n = pat.n
    offL = sym.L_entries != sym.L_rows
    pkeys = np.concatenate([(sym.L_rows * n + sym.L_entries)[offL], sym.U_rows * n + sym.U_entries])
    pkeys.sort()
    a = np.zeros(pkeys.shape[0], dtype=wide)
    a[np.searchsorted(pkeys, pat.rows * n + pat.entries)] = A_values.astype(wide)
    acc, scale, m = np.zeros(pkeys.shape[0], dtype=wide), np.zeros(pkeys.shape[0]), np.zeros(pkeys.shape[0], dtype=np.int64)
    ulen = np.diff(sym.U_row_map)
    Lw, Uw = L_values.astype(wide), U_values.astype(wide)
    step = 1 << 14                                             # L entries per pass: bounds the expansion
    for p0 in range(0, sym.nnzL, step):
        p = np.arange(p0, min(p0 + step, sym.nnzL))
        k = sym.L_entries[p].astype(np.int64)
        cnt = ulen[k]
        start = np.repeat(sym.U_row_map[k] - (np.cumsum(cnt) - cnt), cnt)
        q = start + np.arange(int(cnt.sum()))                  # every entry of U row k, for every (i,k) of the pass
        key = np.repeat(sym.L_rows[p], cnt) * n + sym.U_entries[q]
        pos = np.minimum(np.searchsorted(pkeys, key), pkeys.shape[0] - 1)
        hit = pkeys[pos] == key
        prod = (np.repeat(Lw[p], cnt) * Uw[q])[hit]
        np.add.at(acc, pos[hit], prod)
        np.add.at(scale, pos[hit], np.abs(prod).astype(np.float64))
        np.add.at(m, pos[hit], 1)
    if pkeys.shape[0] == 0:
        return 0.0
    r = np.abs(a - acc).astype(np.float64)
    bound = 2.0 * (m + 2) * u * scale
    worst = float((r / bound).max())
    print("%r %s: largest |A - LU| / bound on the pattern = %.3g" % (pat, np.dtype(dtype).name, worst))
    assert (r <= bound).all(), "%r %s: identity above the bound at %d positions, worst ratio %.3g" % (pat, np.dtype(dtype).name, int((r > bound).sum()), worst)
    return worst


def _crs(n, rows, cols, shuffled, rng):
    key = rng.random(cols.shape[0]) if shuffled else cols
    order = np.lexsort((key, rows))
    row_map = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=row_map[1:])
    return row_map, cols[order].astype(np.int32)


def _variants(name, n, rows, cols, seed, diagonal=True):
    """rows, cols: the COO pattern of the off-diagonal entries (repetitions are merged)"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    if diagonal:
        rows, cols = np.concatenate([rows, np.arange(n, dtype=np.int64)]), np.concatenate([cols, np.arange(n, dtype=np.int64)])
    key = np.unique(rows * max(n, 1) + cols)
    rows, cols = key // max(n, 1), key % max(n, 1)
    out = []
    for k, shuffled in enumerate((False, True)):
        rm, ent = _crs(n, rows, cols, shuffled, np.random.default_rng(seed + 10 * k))
        out.append(Pattern(name, n, shuffled, rm, ent, seed + 10 * k))
    return out


def _random_rows(n, max_off, seed):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, max_off + 1, n)
    rows = np.repeat(np.arange(n, dtype=np.int64), cnt)
    cols = (rng.random(rows.shape[0]) * n).astype(np.int64)   # anywhere in the row; a hit on the diagonal merges with it
    return rows, cols


def lattice(nx, ny, nz, points):
    """off-diagonal COO pattern of the 27-point or 7-point stencil on an nx x ny x nz lattice, x fastest"""
    i = np.arange(nx * ny * nz, dtype=np.int64)
    x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
    rows, cols = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx, dy, dz) == (0, 0, 0) or (points == 7 and abs(dx) + abs(dy) + abs(dz) != 1):
                    continue
                ok = (x + dx >= 0) & (x + dx < nx) & (y + dy >= 0) & (y + dy < ny) & (z + dz >= 0) & (z + dz < nz)
                rows.append(i[ok]); cols.append((i + dx + nx * (dy + ny * dz))[ok])
    return np.concatenate(rows), np.concatenate(cols)


@functools.lru_cache(maxsize=None)
def cases(small):
    """{name: [sorted, shuffled]}; built once per process and never modified"""
    out = {}
    n = 70 if small else 1000
    out["a"] = _variants("a", n, [], [], 100)
    n = 200 if small else 20000
    out["b"] = _variants("b", n, *_random_rows(n, 3, 200), 200)
    n, long_rows = (80, 150) if small else (600, 300)
    out["c"] = _variants("c", n, *_random_rows(n, long_rows, 300), 300)
    n = 24 if small else 3000
    i = np.arange(1, n)
    out["d"] = _variants("d", n, np.concatenate([i, i - 1]), np.concatenate([i - 1, i]), 400)
    dims = (6, 5, 4) if small else (12, 12, 12)
    out["e27"] = _variants("e27", dims[0] * dims[1] * dims[2], *lattice(*dims, 27), 500)
    out["e7"] = _variants("e7", dims[0] * dims[1] * dims[2], *lattice(*dims, 7), 550)
    out["f0"] = _variants("f0", 0, [], [], 600)
    out["f1"] = _variants("f1", 1, [], [], 700)
    return out


def all_patterns(small, names=None):
    return [p for k, v in cases(small).items() if names is None or k in names for p in v]


def exact_cases(small):
    """(pattern, fill_lev) of the exact class: every pattern at k = 0, b and d at k = 1, 2"""
    return [(p, k) for name, v in cases(small).items() for p in v for k in ((0, 1, 2) if name in ("b", "d") else (0,))]


@functools.lru_cache(maxsize=None)
def g_cases():
    """[(name, pattern, A_values, fill_lev)] for the 1e6 rule (numeric_impl.hpp:528-534); the expected factors come from
    reference_numeric (every operation of both is exact).  g-missing: a 6 x 6 matrix whose rows 2, 4 and 5 store no diagonal; row 2's
    is filled by an update (-6), rows 4 and 5 end with U(i,i) == 0 exactly.  g-cancel: a_11 - l_10 u_01 = 4 - 2 * 2 cancels to zero."""
    rows = np.array([0, 0, 1, 1, 1, 2, 2, 3, 3, 4, 5], dtype=np.int64)
    cols = np.array([0, 1, 0, 1, 2, 1, 3, 2, 3, 5, 3], dtype=np.int64)
    vals = np.array([2.0, 1.0, 4.0, 3.0, 2.0, 3.0, 1.0, 12.0, 5.0, 1.0, 14.0])
    missing = Pattern("g-missing", 6, False, *_crs(6, rows, cols, False, None), 800)
    rows = np.array([0, 0, 1, 1, 1, 2, 2], dtype=np.int64)
    cols = np.array([0, 1, 0, 1, 2, 1, 2], dtype=np.int64)
    cancel = Pattern("g-cancel", 3, False, *_crs(3, rows, cols, False, None), 900)
    return [("g-missing", missing, vals, 1), ("g-cancel", cancel, np.array([1.0, 2.0, 2.0, 4.0, 1.0, 3.0, 5.0]), 0)]


# ---------------------------------------------------------------------------------------------------------------------------------
# drivers shared by the emulator and the GPU tests: everything goes through the package's public names and a Backend

class Factored:
    """a pattern on the backend's device with an analysed SPILUK handle and the graphs of L and U"""

    def __init__(self, kk, be, pat, fill_lev, offset_dtype=np.int32, slack=0):
        self.kk, self.be, self.pat, self.fill_lev = kk, be, pat, fill_lev
        self.sym = sym = pat.symbolic(fill_lev)
        self.A_row_map = be.from_numpy(pat.row_map.astype(offset_dtype))
        self.A_entries = be.from_numpy(pat.entries)
        self.L_row_map = be.from_numpy(np.full(pat.n + 1, -1, dtype=offset_dtype))
        self.U_row_map = be.from_numpy(np.full(pat.n + 1, -1, dtype=offset_dtype))
        self.L_entries = be.from_numpy(np.full(sym.nnzL + slack, -1, dtype=np.int32))
        self.U_entries = be.from_numpy(np.full(sym.nnzU + slack, -1, dtype=np.int32))
        self.kh = kk.KokkosKernelsHandle(be)
        self.kh.create_spiluk_handle("SEQLVLSCHD_TP1", pat.n, sym.nnzL + slack, sym.nnzU + slack)
        self.ih = self.kh.get_spiluk_handle()
        self.symbolic(fill_lev)

    def symbolic(self, fill_lev):
        self.fill_lev, self.sym = fill_lev, self.pat.symbolic(fill_lev)
        self.kk.spiluk_symbolic(self.kh, fill_lev, self.A_row_map, self.A_entries, self.L_row_map, self.L_entries, self.U_row_map, self.U_entries)

    def numeric(self, A_values, dtype):
        """(L_values, U_values) over NaN-seeded buffers, as host arrays"""
        be = self.be
        a = be.from_numpy(A_values.astype(dtype))
        lv = be.from_numpy(np.full(self.L_entries.shape[0], np.nan, dtype=dtype))
        uv = be.from_numpy(np.full(self.U_entries.shape[0], np.nan, dtype=dtype))
        self.kk.spiluk_numeric(self.kh, self.fill_lev, self.A_row_map, self.A_entries, a, self.L_row_map, self.L_entries, lv, self.U_row_map,
                               self.U_entries, uv)
        return be.to_numpy(lv)[:self.sym.nnzL], be.to_numpy(uv)[:self.sym.nnzU]

    def close(self):
        self.kh.destroy_spiluk_handle()


def check_symbolic(f):
    sym, ih, be = f.sym, f.ih, f.be
    assert ih.is_symbolic_complete() and ih.get_nrows() == sym.n
    assert (ih.get_nnzL(), ih.get_nnzU()) == (sym.nnzL, sym.nnzU)
    assert np.array_equal(be.to_numpy(f.L_row_map), sym.L_row_map) and np.array_equal(be.to_numpy(f.U_row_map), sym.U_row_map)
    assert np.array_equal(be.to_numpy(f.L_entries)[:sym.nnzL], sym.L_entries) and np.array_equal(be.to_numpy(f.U_entries)[:sym.nnzU], sym.U_entries)
    assert (be.to_numpy(f.L_entries)[sym.nnzL:] == -1).all() and (be.to_numpy(f.U_entries)[sym.nnzU:] == -1).all()
    assert ih.get_num_levels() == sym.num_levels and ih.get("max_level_rows") == sym.max_level_rows
    assert np.array_equal(ih.export("level_list"), sym.level_list)
    assert np.array_equal(ih.export("level_ptr"), sym.level_ptr)
    assert np.array_equal(ih.export("level_idx"), sym.level_idx)
    assert ih.get("plan_bytes") <= 64 * (sym.n + sym.nnzL + sym.nnzU) + 4096


def check_exact(f, dtype):
    A, L, U = f.pat.exact(f.fill_lev)
    lv, uv = f.numeric(A, dtype)
    assert lv.dtype == np.dtype(dtype) and uv.dtype == np.dtype(dtype)
    assert np.array_equal(lv, L.astype(dtype)), "%r k=%d %s: L differs at %d entries" % (f.pat, f.fill_lev, np.dtype(dtype), int((lv != L).sum()))
    assert np.array_equal(uv, U.astype(dtype)), "%r k=%d %s: U differs at %d entries" % (f.pat, f.fill_lev, np.dtype(dtype), int((uv != U).sum()))


def check_knob_sweep(kk, be, pat, fill_lev, dtypes, offset_dtype, alternate=False):
    """exact factors and the launch counts for every combination of lanes_per_row, chain_rows and chain_levels; with `alternate` every
    combination runs one of the value types, in turn (each lane count still meets each of them under four chain settings)"""
    f = Factored(kk, be, pat, fill_lev, offset_dtype)
    turn = 0
    for lanes in LANES:
        for chain_rows in CHAIN_ROWS:
            for chain_levels in CHAIN_LEVELS:
                f.ih.set("lanes_per_row", lanes); f.ih.set("chain_rows", chain_rows); f.ih.set("chain_levels", chain_levels)
                got = (f.ih.get("launches"), f.ih.get("chain_launches"), f.ih.get("chained_levels"))
                assert got == expected_launches(f.sym.level_ptr, chain_rows, chain_levels), (pat, lanes, chain_rows, chain_levels)
                for dtype in (dtypes[turn % len(dtypes)],) if alternate else dtypes:
                    check_exact(f, dtype)
                turn += 1
    f.close()
