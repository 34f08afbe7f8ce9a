"""Generated inputs of the sparse triangular solve tests (CPU only; shared by test_emu_sptrsv.py and test_gpu_sptrsv.py).

Cases (numpy.random.default_rng with fixed seeds; `small` cuts them to emulator size, n <= 300):
  a  diagonal only
  b  random lower, 0-3 off-diagonal entries per row drawn (with repetition) from all earlier rows: few, wide levels and a narrow tail
  c  long rows, up to 300 off-diagonal entries: every lanes-per-row value, and rows beyond one pass of 64 lanes
  d  bidiagonal: one row per level, all chained, more levels than the default chain_levels
  e  the triangle, diagonal included, of the 27-point lattice
  f  n = 0 and n = 1
Every case comes as a lower triangle and as its transpose (upper), with the entries of every row sorted by column and shuffled.

Level sets: a restatement of the reference's sequential loops (sparse/impl/KokkosSparse_sptrsv_symbolic_impl.hpp:194-214 lower,
:617-639 upper).

Two value classes:
  exact    off-diagonal integers 1 <= |a| <= 4, diagonals from {0.5, 1, 2, 4, -1, -2}, a known integer solution x* in [-8, 8] and
           b = A x* evaluated in int64 (on 2 A, halved).  Every partial sum of every row is an integer below 2^24 (asserted), so
           every order of summation gives x* bit for bit, in fp64 and in fp32.
  rounded  off-diagonals uniform in (-1, 1), |diagonal| between 1x and 2x of (1 + sum |off-diagonal|), b uniform in (-1, 1).
"""
import functools

import numpy as np

ALGORITHMS = {"SEQLVLSCHD_RP": 0, "SEQLVLSCHD_TP1": 1, "SEQLVLSCHD_TP1CHAIN": 2, "SPTRSV_CUSPARSE": 3}
LANES = (0, 1, 2, 4, 8, 16, 32, 64)
CHAIN_ROWS = (0, 1, 64, 256)
CHAIN_LEVELS = (2, 1024)


class Triangle:
    """one CRS triangle (row_map int64, entries int32) with its reference level sets and both value classes"""

    def __init__(self, name, n, lower, shuffled, row_map, entries, seed):
        self.name, self.n, self.lower, self.shuffled = name, n, lower, shuffled
        self.row_map, self.entries = row_map, entries
        self._seed = seed

    def __repr__(self):
        return "%s-%s-%s" % (self.name, "lower" if self.lower else "upper", "shuffled" if self.shuffled else "sorted")

    @functools.cached_property
    def rows(self):
        return np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.row_map))

    @functools.cached_property
    def levels(self):
        return reference_levels(self.n, self.row_map, self.entries, self.lower)

    @functools.cached_property
    def exact(self):
        """(values, b, xstar) as float64 arrays holding numbers that fp32 represents too"""
        rng = np.random.default_rng(self._seed + 1)
        rows, cols, n = self.rows, self.entries.astype(np.int64), self.n
        nnz = cols.shape[0]
        off = rng.integers(1, 5, nnz) * rng.choice([-1, 1], nnz)
        dia = rng.choice([1, 2, 4, 8, -2, -4], nnz)             # twice the diagonal values {0.5, 1, 2, 4, -1, -2}
        twice = np.where(rows == cols, dia, 2 * off).astype(np.int64)
        xstar = rng.integers(-8, 9, n).astype(np.int64)
        b2 = np.zeros(n, dtype=np.int64)
        np.add.at(b2, rows, twice * xstar[cols])
        bound = np.zeros(n, dtype=np.int64)
        np.add.at(bound, rows, np.abs(twice) * np.abs(xstar[cols]))
        assert n == 0 or bound.max() < 2 ** 24, "partial sums of %r are not exact in fp32" % self
        return twice / 2.0, b2 / 2.0, xstar.astype(np.float64)

    @functools.cached_property
    def rounded(self):
        """(values, b) in float64"""
        rng = np.random.default_rng(self._seed + 2)
        rows, cols, n = self.rows, self.entries.astype(np.int64), self.n
        nnz = cols.shape[0]
        val = rng.uniform(-1.0, 1.0, nnz)
        isdiag = rows == cols
        s = np.zeros(n)
        np.add.at(s, rows[~isdiag], np.abs(val[~isdiag]))
        d = (1.0 + s) * rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
        val[isdiag] = d[rows[isdiag]]
        return val, rng.uniform(-1.0, 1.0, n)


def reference_levels(n, row_map, entries, lower):
    """(level_list, nodes_per_level, nodes_grouped_by_level) as the reference's symbolic phase computes them: rows in solve order,
    level(i) = 1 + max level(col) over the off-diagonal columns (symbolic_impl.hpp:194-214; upper, rows descending, :617-639);
    rows ascending inside a level"""
    level = np.zeros(n, dtype=np.int32)
    for i in (range(n) if lower else range(n - 1, -1, -1)):
        c = entries[row_map[i]:row_map[i + 1]]
        c = c[c != i]
        level[i] = 1 + (level[c].max() if c.shape[0] else 0)
    nlev = int(level.max()) if n else 0
    per_level = np.bincount(level, minlength=nlev + 1)[1:].astype(np.int32)
    grouped = np.argsort(level, kind="stable").astype(np.int32)
    return level, per_level, grouped


def expected_launches(nodes_per_level, algorithm, chain_rows, chain_levels):
    """(launches, chain_launches, chained_levels) of one solve: one launch per level, except that under SEQLVLSCHD_TP1CHAIN every
    run of two or more consecutive levels with at most chain_rows rows each goes into ceil(run / chain_levels) chain launches"""
    launches = chain_launches = chained = 0
    chaining = algorithm == ALGORITHMS["SEQLVLSCHD_TP1CHAIN"] and chain_rows > 0
    L, l = len(nodes_per_level), 0
    while l < L:
        run = 0
        while chaining and l + run < L and nodes_per_level[l + run] <= chain_rows:
            run += 1
        if run < 2:
            launches += 1
            l += 1
            continue
        pieces = -(-run // chain_levels)
        launches += pieces
        chain_launches += pieces
        chained += run
        l += run
    return launches, chain_launches, chained


def _crs(n, rows, cols, shuffled, rng):
    key = rng.random(cols.shape[0]) if shuffled else cols
    order = np.lexsort((key, rows))
    row_map = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=row_map[1:])
    return row_map, cols[order].astype(np.int32)


def _variants(name, n, rows, cols, seed):
    """rows, cols: the COO pattern of the LOWER triangle, off-diagonal entries only (repetitions allowed)"""
    rows = np.concatenate([np.asarray(rows, dtype=np.int64), np.arange(n, dtype=np.int64)])
    cols = np.concatenate([np.asarray(cols, dtype=np.int64), np.arange(n, dtype=np.int64)])
    assert (cols <= rows).all()
    out = []
    for k, (lower, shuffled) in enumerate(((True, False), (True, True), (False, False), (False, True))):
        r, c = (rows, cols) if lower else (cols, rows)
        rm, ent = _crs(n, r, c, shuffled, np.random.default_rng(seed + 10 * k))
        out.append(Triangle(name, n, lower, shuffled, rm, ent, seed + 10 * k))
    return out


def _random_lower(n, max_off, seed):
    rng = np.random.default_rng(seed)
    cnt = np.minimum(rng.integers(0, max_off + 1, n), np.arange(n))  # row i has i earlier rows to draw from
    rows = np.repeat(np.arange(n, dtype=np.int64), cnt)
    cols = (rng.random(rows.shape[0]) * rows).astype(np.int64)       # uniform over the earlier rows [0, row)
    return rows, cols


def lattice27_lower(nx, ny, nz):
    """off-diagonal COO pattern of the lower triangle of the 27-point stencil on an nx x ny x nz lattice, x fastest"""
    i = np.arange(nx * ny * nz, dtype=np.int64)
    x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
    rows, cols = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = (x + dx >= 0) & (x + dx < nx) & (y + dy >= 0) & (y + dy < ny) & (z + dz >= 0) & (z + dz < nz)
                j = i + dx + nx * (dy + ny * dz)
                ok &= j < i
                rows.append(i[ok]); cols.append(j[ok])
    return np.concatenate(rows), np.concatenate(cols)


@functools.lru_cache(maxsize=None)
def cases(small):
    """{name: [lower-sorted, lower-shuffled, upper-sorted, upper-shuffled]}; built once per process and never modified"""
    out = {}
    n = 70 if small else 1000
    out["a"] = _variants("a", n, [], [], 100)
    n = 200 if small else 20000
    out["b"] = _variants("b", n, *_random_lower(n, 3, 200), 200)
    n, long_rows = (80, 150) if small else (600, 300)
    out["c"] = _variants("c", n, *_random_lower(n, long_rows, 300), 300)
    n = 24 if small else 3000
    out["d"] = _variants("d", n, np.arange(1, n), np.arange(0, n - 1), 400)
    dims = (6, 5, 4) if small else (12, 12, 12)
    out["e"] = _variants("e", dims[0] * dims[1] * dims[2], *lattice27_lower(*dims), 500)
    out["f0"] = _variants("f0", 0, [], [], 600)
    out["f1"] = _variants("f1", 1, [], [], 700)
    return out


def all_triangles(small, names=None):
    return [t for k, v in cases(small).items() if names is None or k in names for t in v]


# ---------------------------------------------------------------------------------------------------------------------------------
# drivers shared by the emulator and the GPU tests: everything goes through the package's public names and a Backend

class Analysed:
    """a triangle on the backend's device with an analysed SPTRSV handle"""

    def __init__(self, kk, be, tri, algo="SEQLVLSCHD_TP1CHAIN", offset_dtype=np.int32):
        self.kk, self.be, self.tri = kk, be, tri
        self.row_map = be.from_numpy(tri.row_map.astype(offset_dtype))
        self.entries = be.from_numpy(tri.entries)
        self.kh = kk.KokkosKernelsHandle(be)
        self.kh.create_sptrsv_handle(algo, tri.n, tri.lower)
        self.th = self.kh.get_sptrsv_handle()
        kk.sptrsv_symbolic(self.kh, self.row_map, self.entries)

    def solve(self, values, b, dtype, alias=False):
        """x over a NaN-seeded buffer (or over b itself), as a host array"""
        be = self.be
        v = be.from_numpy(values.astype(dtype))
        if alias:
            x = be.from_numpy(b.astype(dtype))
            self.kk.sptrsv_solve(self.kh, self.row_map, self.entries, v, x, x)
        else:
            x = be.from_numpy(np.full(self.tri.n, np.nan, dtype=dtype))
            self.kk.sptrsv_solve(self.kh, self.row_map, self.entries, v, be.from_numpy(b.astype(dtype)), x)
        return be.to_numpy(x)

    def close(self):
        self.kh.destroy_sptrsv_handle()


def check_level_sets(an):
    tri, th = an.tri, an.th
    level, per_level, grouped = tri.levels
    assert th.is_symbolic_complete() and th.get_nrows() == tri.n and th.is_lower_tri() == tri.lower and th.is_upper_tri() != tri.lower
    assert th.get_num_levels() == per_level.shape[0]
    assert th.get("max_level_rows") == (int(per_level.max()) if per_level.shape[0] else 0)
    assert np.array_equal(th.export("level_list"), level)
    assert np.array_equal(th.export("nodes_per_level"), per_level)
    assert np.array_equal(th.export("nodes_grouped_by_level"), grouped)


def check_exact(an, dtype, alias=False):
    values, b, xstar = an.tri.exact
    x = an.solve(values, b, dtype, alias=alias)
    assert x.dtype == np.dtype(dtype)
    assert np.array_equal(x, xstar.astype(dtype)), "%r %s: x differs from x* in %d rows" % (an.tri, np.dtype(dtype), int((x != xstar).sum()))


def check_knob_sweep(kk, be, tri, dtypes, offset_dtype, algos=("SEQLVLSCHD_RP", "SEQLVLSCHD_TP1", "SEQLVLSCHD_TP1CHAIN")):
    """exact values and the launch counts for every combination of algorithm, lanes_per_row, chain_rows and chain_levels"""
    per_level = tri.levels[1]
    for algo in algos:
        aid = ALGORITHMS[algo]
        an = Analysed(kk, be, tri, algo, offset_dtype)
        for lanes in LANES:
            for chain_rows in CHAIN_ROWS:
                for chain_levels in CHAIN_LEVELS:
                    an.th.set("lanes_per_row", lanes); an.th.set("chain_rows", chain_rows); an.th.set("chain_levels", chain_levels)
                    got = (an.th.get("launches"), an.th.get("chain_launches"), an.th.get("chained_levels"))
                    assert got == expected_launches(per_level, aid, chain_rows, chain_levels), (tri, algo, lanes, chain_rows, chain_levels)
                    for dtype in dtypes:
                        check_exact(an, dtype)
        an.close()


def residual_check(tri, values, b, x, dtype):
    """|r_i| <= 2 (k_i + 2) u sum_j |a_ij| |x_j| for r = b - A x evaluated row by row in the next wider format: the backward-error bound
    of substitution for any order of evaluation (Higham, Accuracy and Stability of Numerical Algorithms, Thm 8.5); the factor 2 covers
    the gamma denominator and the residual's own rounding.  values, b, x are what the solver saw and gave, in `dtype`.
    Returns the largest ratio |r_i| / bound_i."""
    wide, u = (np.longdouble, 2.0 ** -53) if np.dtype(dtype) == np.dtype(np.float64) else (np.float64, 2.0 ** -24)
    assert values.dtype == np.dtype(dtype) and b.dtype == np.dtype(dtype) and x.dtype == np.dtype(dtype)
    assert np.isfinite(x).all()
    rows, cols = tri.rows, tri.entries.astype(np.int64)
    prod = values.astype(wide) * x.astype(wide)[cols]
    ax = np.zeros(tri.n, dtype=wide)
    np.add.at(ax, rows, prod)
    r = np.abs(b.astype(wide) - ax).astype(np.float64)
    scale = np.zeros(tri.n)
    np.add.at(scale, rows, np.abs(prod).astype(np.float64))
    bound = 2.0 * (np.diff(tri.row_map) + 2) * u * scale
    worst = float((r / bound).max())
    print("%r %s: largest residual / bound = %.3g" % (tri, np.dtype(dtype).name, worst))
    assert (r <= bound).all(), "%r %s: residual above the bound in %d rows, worst ratio %.3g" % (tri, np.dtype(dtype).name, int((r > bound).sum()), worst)
    return worst
