"""Generated inputs of the multicolor Gauss-Seidel tests (CPU only; shared by test_emu_gauss_seidel.py and test_gpu_gauss_seidel.py).

Cases (numpy.random.default_rng with fixed seeds; `small` cuts them to emulator size, n <= 300):
  a      diagonal only: one colour
  b      path graph (tridiagonal), computed colours;  b-rb: the caller's red-black colours
  c      the 27-point lattice, computed colours;  c-par: the 8 parity colours supplied
  d      random symmetric graph, 0-3 off-diagonal entries per row drawn from all rows, then symmetrised
  e      long rows: a few rows with up to 300 off-diagonals, the others 0-3, symmetrised: every lanes-per-row value, rows beyond one
         pass of 64 lanes, long_row_threshold 0 and 64
  f      strictly lower-triangular pattern plus the diagonal, declared is_graph_symmetric=False: A's own rows show no upper neighbour
  g      rectangular, num_cols = num_rows + 37, ghost columns in about a third of the rows
  h0 h1  n = 0 and n = 1
  i      n = 200 path with supplied colours cycling through 70 values: at most 3 rows per colour, every colour chained
Every case comes with the entries of every row sorted by column and shuffled.

The colouring restated: sequential greedy (smallest colour no coloured neighbour holds) over the rows in descending (h(i), i), h the
32-bit mix that include/kkamd.h states.  The sweep restated from the reference's update (sparse/impl/KokkosSparse_gauss_seidel_impl.hpp:
159-179: sum = y_i - sum_j a_ij x_j over the whole row, x_i += omega * sum * inv_diag_i) in the order of :1520-1560 (colours 1..C forward,
C..1 backward).

Two value classes:
  exact    off-diagonal integers 1 <= |a| <= 4, diagonals from {0.5, 1, 2, 4, -1, -2}, omega from {1, 0.5, 1.5}, an integer x0 in
           [-8, 8], a chosen integer result x1 of one sweep (x1 - x0 a multiple of 3 for omega = 1.5), and
           y_i = d_i (x1_i - x0_i) / omega + sum_j a_ij xin_j in int64 on doubled values, xin_j = x1_j for the columns swept before row i
           and x0_j otherwise (ghost columns and the diagonal included).  sum_j |a_ij xin_j| + |y_i| < 2^24 is asserted, so every order
           of summation gives x1 bit for bit, in fp64 and in fp32.
  rounded  off-diagonals uniform in (-1, 1), |a_ii| between 1x and 2x of 1 + sum |off-diagonal|, y and x0 uniform in (-1, 1).
"""
import functools

import numpy as np
import pytest

ALGORITHMS = ("GS_DEFAULT", "GS_PERMUTED", "GS_TEAM")
DIRECTIONS = ("forward", "backward")
OMEGAS = (1.0, 0.5, 1.5)
THRESHOLDS = (0, 64)


def gs_hash(i):
    """h of include/kkamd.h on an array of row numbers, in uint32 arithmetic"""
    x = np.asarray(i).astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    x = x ^ (x >> np.uint32(16))
    return x


class Case:
    """one CRS matrix pattern (row_map int64, entries int32; num_cols >= n) with how symbolic is to be called"""

    def __init__(self, name, n, ncols, shuffled, row_map, entries, symmetric, supplied, seed):
        self.name, self.n, self.ncols, self.shuffled = name, n, ncols, shuffled
        self.row_map, self.entries, self.symmetric, self.supplied = row_map, entries, symmetric, supplied
        self._seed = seed

    def __repr__(self):
        return "%s-%s" % (self.name, "shuffled" if self.shuffled else "sorted")

    @functools.cached_property
    def rows(self):
        return np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.row_map))

    @functools.cached_property
    def row_len(self):
        return np.diff(self.row_map)

    @functools.cached_property
    def adjacency(self):
        """(ptr, adj): the symmetrised graph of the leading n x n block without the diagonal, neighbours ascending"""
        r, c = self.rows, self.entries.astype(np.int64)
        keep = (c < self.n) & (c != r)
        r, c = r[keep], c[keep]
        key = np.unique(np.concatenate([r * max(self.n, 1) + c, c * max(self.n, 1) + r]))
        rr, cc = key // max(self.n, 1), key % max(self.n, 1)
        ptr = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(np.bincount(rr, minlength=self.n), out=ptr[1:])
        return ptr, cc

    @functools.cached_property
    def greedy(self):
        """(colors int32 1-based, rounds): the sequential greedy colouring in descending (h(i), i); rounds = how many Jones-Plassmann
        rounds give it: a row is coloured in the round after the last of its higher-priority neighbours"""
        n = self.n
        ptr, adj = self.adjacency
        h = gs_hash(np.arange(n))
        order = np.lexsort((np.arange(n), h))[::-1]
        colors = np.zeros(n, dtype=np.int32)
        rnd = np.zeros(n, dtype=np.int64)
        for v in order:
            nb = adj[ptr[v]:ptr[v + 1]]
            done = nb[colors[nb] > 0]
            used = set(colors[done].tolist())
            c = 1
            while c in used:
                c += 1
            colors[v] = c
            rnd[v] = 1 + (rnd[done].max() if done.shape[0] else 0)
        return colors, int(rnd.max()) if n else 0

    @functools.cached_property
    def colors(self):
        """the colours symbolic is expected to hold: the caller's, or the greedy ones"""
        return self.supplied if self.supplied is not None else self.greedy[0]

    def grouping(self, threshold):
        """(color_xadj, color_adj, old_to_new, long_begin): rows by colour, ascending inside a colour, the rows with more than
        threshold entries (threshold > 0) at the end of their colour, ascending"""
        colors = self.colors
        is_long = (self.row_len > threshold) if threshold > 0 else np.zeros(self.n, dtype=bool)
        adj = np.lexsort((np.arange(self.n), is_long, colors)).astype(np.int32)
        C = int(colors.max()) if self.n else 0
        xadj = np.zeros(C + 1, dtype=np.int32)
        np.cumsum(np.bincount(colors, minlength=C + 1)[1:], out=xadj[1:])
        o2n = np.zeros(self.n, dtype=np.int32)
        o2n[adj] = np.arange(self.n, dtype=np.int32)
        nlong = np.bincount(colors[is_long], minlength=C + 1)[1:] if self.n else np.zeros(0, dtype=np.int64)
        return xadj, adj, o2n, xadj[1:] - nlong

    def order(self, direction):
        """position of every row in the sweep (smaller = swept earlier)"""
        return self.colors.astype(np.int64) if direction == "forward" else -self.colors.astype(np.int64)

    @functools.lru_cache(maxsize=None)
    def exact(self, direction, omega, zero_x=False):
        """(values, x0, y, x1) as float64 arrays holding numbers that fp32 represents too: one sweep in `direction` maps x0 to x1"""
        rng = np.random.default_rng(self._seed + 1 + 7 * DIRECTIONS.index(direction) + 3 * OMEGAS.index(omega))
        rows, cols, n = self.rows, self.entries.astype(np.int64), self.n
        nnz = cols.shape[0]
        off = rng.integers(1, 5, nnz) * rng.choice([-1, 1], nnz)
        dia = rng.choice([1, 2, 4, 8, -2, -4], nnz)            # twice the diagonal values {0.5, 1, 2, 4, -1, -2}
        twice = np.where(rows == cols, dia, 2 * off).astype(np.int64)
        x0 = rng.integers(-8, 9, self.ncols).astype(np.int64)
        if zero_x:
            x0[:] = 0
        step = rng.integers(-2, 3, n) * 3 if omega == 1.5 else rng.integers(-6, 7, n)
        x1 = x0.copy()
        x1[:n] += step
        num, den = {1.0: (1, 1), 0.5: (2, 1), 1.5: (2, 3)}[omega]          # 1 / omega
        order = self.order(direction)
        earlier = np.zeros(nnz, dtype=bool)
        inblock = cols < n
        earlier[inblock] = order[cols[inblock]] < order[rows[inblock]]
        xin = np.where(earlier, x1[cols], x0[cols])
        y2 = np.zeros(n, dtype=np.int64)
        np.add.at(y2, rows, twice * xin)
        d2 = np.zeros(n, dtype=np.int64)
        np.add.at(d2, rows[rows == cols], twice[rows == cols])
        assert (step * num % den == 0).all()
        y2 += d2 * (step * num // den)
        bound = np.zeros(n, dtype=np.int64)
        np.add.at(bound, rows, np.abs(twice * xin))
        assert n == 0 or (bound + np.abs(y2)).max() < 2 * 2 ** 24, "partial sums of %r are not exact in fp32" % self
        return twice / 2.0, x0.astype(np.float64), y2 / 2.0, x1.astype(np.float64)

    @functools.cached_property
    def rounded(self):
        """(values, x0, y) in float64"""
        rng = np.random.default_rng(self._seed + 2)
        rows, cols, n = self.rows, self.entries.astype(np.int64), self.n
        val = rng.uniform(-1.0, 1.0, cols.shape[0])
        isdiag = rows == cols
        s = np.zeros(n)
        np.add.at(s, rows[~isdiag], np.abs(val[~isdiag]))
        d = (1.0 + s) * rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)
        val[isdiag] = d[rows[isdiag]]
        return val, rng.uniform(-1.0, 1.0, self.ncols), rng.uniform(-1.0, 1.0, n)


def reference_sweep(case, values, x, y, omega, direction, dtype):
    """one sequential sweep in `dtype`, in place on x and returned: rows colour by colour (ascending inside a colour; rows of one colour
    do not read one another), sum = y_i - sum_j a_ij x_j entry by entry over the whole row, x_i += omega * sum * (1 / a_ii)"""
    dt = np.dtype(dtype).type
    xadj, adj, _, _ = case.grouping(0)
    C = xadj.shape[0] - 1
    omega = dt(omega)
    for c in (range(C) if direction == "forward" else range(C - 1, -1, -1)):
        for i in adj[xadj[c]:xadj[c + 1]]:
            s, e = case.row_map[i], case.row_map[i + 1]
            cols = case.entries[s:e]
            total = dt(y[i])
            for a, xj in zip(values[s:e], x[cols]):
                total = dt(total - dt(dt(a) * dt(xj)))
            inv = dt(dt(1) / dt(values[s:e][cols == i][0]))
            x[i] = dt(x[i] + dt(dt(omega * total) * inv))
    return x


def expected_plan(case, threshold, chain_rows, chain_levels):
    """(launches, chain_launches, chained_levels, tail_launches) of one sweep: one launch per colour, except that every run of two or
    more consecutive colours with at most chain_rows rows each goes into ceil(run / chain_levels) chain launches; a colour outside a
    chain that has long rows launches them separately (counted in tail_launches, not in launches)"""
    xadj, _, _, long_begin = case.grouping(threshold)
    sizes = np.diff(xadj)
    launches = chain_launches = chained = tails = 0
    L, l = len(sizes), 0
    while l < L:
        run = 0
        while chain_rows > 0 and l + run < L and sizes[l + run] <= chain_rows:
            run += 1
        if run < 2:
            launches += 1
            tails += int(long_begin[l] < xadj[l + 1])
            l += 1
            continue
        pieces = -(-run // chain_levels)
        launches += pieces
        chain_launches += pieces
        chained += run
        l += run
    return launches, chain_launches, chained, tails


def _crs(n, rows, cols, shuffled, rng):
    key = rng.random(cols.shape[0]) if shuffled else cols
    order = np.lexsort((key, rows))
    row_map = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=row_map[1:])
    return row_map, cols[order].astype(np.int32)


def _variants(name, n, rows, cols, seed, ncols=None, symmetric=True, supplied=None, symmetrise=True):
    """rows, cols: the COO pattern without the diagonal (repetitions allowed, removed here); ghost columns are >= n"""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    ncols = n if ncols is None else ncols
    if symmetrise:
        inner = cols < n
        rows, cols = np.concatenate([rows, cols[inner]]), np.concatenate([cols, rows[inner]])
    keep = rows != cols
    key = np.unique(np.concatenate([rows[keep] * max(ncols, 1) + cols[keep], np.arange(n, dtype=np.int64) * (max(ncols, 1) + 1)]))
    rows, cols = key // max(ncols, 1), key % max(ncols, 1)
    out = []
    for k, shuffled in enumerate((False, True)):
        rm, ent = _crs(n, rows, cols, shuffled, np.random.default_rng(seed + 10 * k))
        out.append(Case(name, n, ncols, shuffled, rm, ent, symmetric, None if supplied is None else np.asarray(supplied, dtype=np.int32), seed + 10 * k))
    return out


def _random_pairs(n, max_off, seed, lower=False):
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, max_off + 1, n)
    if lower:
        cnt = np.minimum(cnt, np.arange(n))
    rows = np.repeat(np.arange(n, dtype=np.int64), cnt)
    cols = (rng.random(rows.shape[0]) * (rows if lower else n)).astype(np.int64)
    return rows, cols


def lattice27(nx, ny, nz):
    """off-diagonal COO pattern of the 27-point stencil on an nx x ny x nz lattice, x fastest, and the 8 parity colours (1-based)"""
    i = np.arange(nx * ny * nz, dtype=np.int64)
    x, y, z = i % nx, (i // nx) % ny, i // (nx * ny)
    rows, cols = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = (x + dx >= 0) & (x + dx < nx) & (y + dy >= 0) & (y + dy < ny) & (z + dz >= 0) & (z + dz < nz) & ((dx, dy, dz) != (0, 0, 0))
                rows.append(i[ok]); cols.append((i + dx + nx * (dy + ny * dz))[ok])
    return np.concatenate(rows), np.concatenate(cols), (1 + x % 2 + 2 * (y % 2) + 4 * (z % 2)).astype(np.int32)


@functools.lru_cache(maxsize=None)
def cases(small):
    """{name: [sorted, shuffled]}; built once per process and never modified"""
    out = {}
    n = 70 if small else 1000
    out["a"] = _variants("a", n, [], [], 100)
    n = 200 if small else 2049
    path = (np.arange(1, n), np.arange(0, n - 1))
    out["b"] = _variants("b", n, *path, 200)
    out["b-rb"] = _variants("b-rb", n, *path, 200, supplied=1 + np.arange(n) % 2)
    dims = (6, 5, 4) if small else (12, 12, 12)
    lr, lc, parity = lattice27(*dims)
    out["c"] = _variants("c", dims[0] * dims[1] * dims[2], lr, lc, 300)
    out["c-par"] = _variants("c-par", dims[0] * dims[1] * dims[2], lr, lc, 300, supplied=parity)
    n = 250 if small else 3000
    out["d"] = _variants("d", n, *_random_pairs(n, 3, 400), 400)
    n, nlong, longest = (300, 3, 150) if small else (1200, 5, 300)
    r, c = _random_pairs(n, 3, 500)
    rng = np.random.default_rng(501)
    for k, row in enumerate(rng.choice(n, nlong, replace=False)):
        cnt = longest if k == 0 else int(rng.integers(70, longest))
        r = np.concatenate([r, np.full(cnt, row)]); c = np.concatenate([c, rng.choice(n, cnt, replace=False)])
    out["e"] = _variants("e", n, r, c, 500)
    n = 200 if small else 1000
    out["f"] = _variants("f", n, *_random_pairs(n, 3, 600, lower=True), 600, symmetric=False, symmetrise=False)
    n = 150 if small else 1000
    r, c = _random_pairs(n, 3, 700)
    rng = np.random.default_rng(701)
    ghost_rows = np.flatnonzero(rng.random(n) < 1.0 / 3.0)
    gr = np.repeat(ghost_rows, rng.integers(1, 3, ghost_rows.shape[0]))
    out["g"] = _variants("g", n, np.concatenate([r, gr]), np.concatenate([c, n + rng.integers(0, 37, gr.shape[0])]), 700, ncols=n + 37)
    out["h0"] = _variants("h0", 0, [], [], 800)
    out["h1"] = _variants("h1", 1, [], [], 900)
    n = 200
    out["i"] = _variants("i", n, np.arange(1, n), np.arange(0, n - 1), 1000, supplied=1 + np.arange(n) % 70)
    return out


def all_cases(small, names=None):
    return [t for k, v in cases(small).items() if names is None or k in names for t in v]


# ---------------------------------------------------------------------------------------------------------------------------------
# drivers shared by the emulator and the GPU tests: everything goes through the package's public names and a Backend

class Smoother:
    """a case on the backend's device with an analysed Gauss-Seidel handle"""

    def __init__(self, kk, be, case, algo="GS_DEFAULT", offset_dtype=np.int32, threshold=0):
        self.kk, self.be, self.case, self.threshold = kk, be, case, threshold
        self.row_map = be.from_numpy(case.row_map.astype(offset_dtype))
        self.entries = be.from_numpy(case.entries)
        self.supplied = None if case.supplied is None else be.from_numpy(case.supplied)
        self.kh = kk.KokkosKernelsHandle(be)
        self.kh.create_gs_handle(algo)
        self.gh = self.kh.get_gs_handle()
        if threshold:
            self.kh.get_point_gs_handle().set_long_row_threshold(threshold)
        self.symbolic()

    def symbolic(self):
        c = self.case
        self.kk.gauss_seidel_symbolic(self.kh, c.n, c.ncols, self.row_map, self.entries, c.symmetric, self.supplied)

    def numeric(self, values, dtype, inverse_diagonal=None):
        c = self.case
        inv = None if inverse_diagonal is None else self.be.from_numpy(inverse_diagonal.astype(dtype))
        self.kk.gauss_seidel_numeric(self.kh, c.n, c.ncols, self.row_map, self.entries, self.be.from_numpy(values.astype(dtype)), inv, c.symmetric)

    def apply_dev(self, direction, values, x, y, init_zero_x=False, update_y=True, omega=1.0, num_iter=1):
        """on arrays of the backend (x in place)"""
        c = self.case
        fn = {"forward": self.kk.forward_sweep_gauss_seidel_apply, "backward": self.kk.backward_sweep_gauss_seidel_apply,
              "symmetric": self.kk.symmetric_gauss_seidel_apply}[direction]
        return fn(self.kh, c.n, c.ncols, self.row_map, self.entries, values, x, y, init_zero_x, update_y, omega, num_iter)

    def apply(self, direction, values, x, y, dtype, numeric=True, **kw):
        """x after the call, as a host array; values, x, y host arrays of any float type.  The numeric phase runs first, as it must
        when the values or their type have changed; numeric=False leaves it to the apply call (a fresh analysis only)"""
        be = self.be
        xd = be.from_numpy(np.asarray(x).astype(dtype))
        if numeric:
            self.numeric(values, dtype)
        self.apply_dev(direction, be.from_numpy(values.astype(dtype)), xd, be.from_numpy(np.asarray(y).astype(dtype)), **kw)
        return be.to_numpy(xd)

    def close(self):
        self.kh.destroy_gs_handle()


def check_coloring(sm):
    """colours, their properties, and the grouped arrays against the restatement"""
    case, gh = sm.case, sm.gh
    colors = gh.export("colors")
    assert gh.is_symbolic_complete() and gh.get("num_rows") == case.n and gh.get("num_cols") == case.ncols
    assert np.array_equal(colors, case.colors), "%r: %d colours differ" % (case, int((colors != case.colors).sum()))
    ptr, adj = case.adjacency
    src = np.repeat(np.arange(case.n), np.diff(ptr))
    assert (colors >= 1).all() and (colors[src] != colors[adj]).all()
    C = int(colors.max()) if case.n else 0
    assert gh.get_num_colors() == C and gh.get_num_levels() == C and set(colors.tolist()) == set(range(1, C + 1))
    if case.supplied is None:
        assert C <= (int(np.diff(ptr).max()) if case.n else 0) + 1
        assert gh.get("coloring_rounds") == case.greedy[1]
    else:
        assert gh.get("coloring_rounds") == 0
    xadj, cadj, o2n, long_begin = case.grouping(sm.threshold)
    assert np.array_equal(gh.export("color_xadj"), xadj)
    assert np.array_equal(gh.export("color_adj"), cadj)
    assert np.array_equal(gh.export("old_to_new"), o2n)
    assert gh.get("long_rows") == int((xadj[1:] - long_begin).sum())
    assert gh.get("max_level_rows") == (int(np.diff(xadj).max()) if C else 0)


def check_exact(sm, dtype, direction, omega=1.0, zero_x=False, numeric=True):
    """one sweep gives the chosen x1 bit for bit; zero_x: init_zero_x over a NaN-seeded x"""
    case = sm.case
    values, x0, y, x1 = case.exact(direction, omega, zero_x)
    xin = np.full(case.ncols, np.nan) if zero_x else x0
    x = sm.apply(direction, values, xin, y, dtype, numeric=numeric, init_zero_x=zero_x, omega=omega)
    assert x.dtype == np.dtype(dtype)
    assert np.array_equal(x, x1.astype(dtype)), "%r %s %s omega %g: x differs from x1 in %d rows" % (
        case, np.dtype(dtype).name, direction, omega, int((x != x1).sum()))


def check_knob_sweep(kk, be, case, dtypes, offset_dtype, lanes, chain_rows_values, chain_levels_values):
    """exact values and the launch counts for every combination of threshold, lanes_per_row, chain_rows and chain_levels"""
    for threshold in THRESHOLDS:
        sm = Smoother(kk, be, case, "GS_DEFAULT", offset_dtype, threshold)
        k = 0
        for lpr in lanes:
            for chain_rows in chain_rows_values:
                for chain_levels in chain_levels_values:
                    sm.gh.set("lanes_per_row", lpr); sm.gh.set("chain_rows", chain_rows); sm.gh.set("chain_levels", chain_levels)
                    got = tuple(sm.gh.get(key) for key in ("launches", "chain_launches", "chained_levels", "tail_launches"))
                    assert got == expected_plan(case, threshold, chain_rows, chain_levels), (case, threshold, lpr, chain_rows, chain_levels)
                    for dtype in dtypes:
                        for direction in DIRECTIONS:
                            check_exact(sm, dtype, direction, OMEGAS[k % 3])
                            k += 1
        sm.close()


def local_bound_check(case, values, x0, y, x, direction, omega, dtype):
    """|x_i - xt_i| <= 2 (k_i + 4) u (|x0_i| + |omega / a_ii| (|y_i| + sum_j |a_ij xin_j|)), xt_i the update of row i evaluated in the next
    wider format from the device's own final x for the columns swept earlier and x0 for the others: the inner-product bound for any
    order of summation (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1) plus the four scalar operations (the
    subtraction from y, the two multiplications, the addition to x; the reciprocal of the diagonal is the +4's spare); the factor 2
    covers the gamma denominator and the wide evaluation's own rounding, as in sptrsv_cases.residual_check.  values, x0, y, x are what
    the kernel saw and gave, in `dtype`.  Returns the largest ratio."""
    wide, u = (np.longdouble, 2.0 ** -53) if np.dtype(dtype) == np.dtype(np.float64) else (np.float64, 2.0 ** -24)
    assert values.dtype == x0.dtype == y.dtype == x.dtype == np.dtype(dtype)
    assert np.isfinite(x).all()
    rows, cols, n = case.rows, case.entries.astype(np.int64), case.n
    order = case.order(direction)
    earlier = np.zeros(cols.shape[0], dtype=bool)
    inblock = cols < n
    earlier[inblock] = order[cols[inblock]] < order[rows[inblock]]
    xin = np.where(earlier, x[cols], x0[cols]).astype(wide)
    prod = values.astype(wide) * xin
    ax = np.zeros(n, dtype=wide)
    np.add.at(ax, rows, prod)
    absax = np.zeros(n, dtype=wide)
    np.add.at(absax, rows, np.abs(prod))
    diag = np.zeros(n, dtype=wide)
    diag[rows[rows == cols]] = values[rows == cols].astype(wide)
    w = wide(omega) / diag
    xt = x0[:n].astype(wide) + w * (y.astype(wide) - ax)
    err = np.abs(x[:n].astype(wide) - xt).astype(np.float64)
    bound = (2.0 * (case.row_len + 4) * u * (np.abs(x0[:n].astype(wide)) + np.abs(w) * (np.abs(y.astype(wide)) + absax))).astype(np.float64)
    worst = float((err / bound).max()) if n else 0.0
    print("%r %s %s: largest error / bound = %.3g" % (case, np.dtype(dtype).name, direction, worst))
    assert (err <= bound).all(), "%r %s: error above the bound in %d rows, worst ratio %.3g" % (case, np.dtype(dtype).name, int((err > bound).sum()), worst)
    return worst


def status_of(kk, fn):
    with pytest.raises(kk.KkamdError) as e:
        fn()
    return e.value.status, str(e.value)


def check_rank2(kk, be, case, nv, layout, dtype):
    """every column of a rank-2 apply equals the rank-1 apply of that column bit for bit; what lies outside the views is untouched"""
    values, _, _ = case.rounded
    rng = np.random.default_rng(nv)
    X0 = rng.uniform(-1, 1, (case.ncols, nv)).astype(dtype); Y = rng.uniform(-1, 1, (case.n, nv)).astype(dtype)
    sm = Smoother(kk, be, case)
    v = be.from_numpy(values.astype(dtype))
    pad = 0 if layout in ("left", "right") else 3

    def view(a):
        """(buffer, view of the buffer holding a) in the layout; the buffer is NaN outside the view"""
        r, c = a.shape
        if layout.endswith("right"):
            host = np.full((r + pad, c + 2 * pad), np.nan, dtype=dtype); host[:r, pad:pad + c] = a
            buf = be.from_numpy(host)
            return buf, buf[:r, pad:pad + c]
        host = np.full((c + pad, r + 2 * pad), np.nan, dtype=dtype); host[:c, pad:pad + r] = a.T
        buf = be.from_numpy(host)
        return buf, buf[:c, pad:pad + r].T

    for direction in ("forward", "symmetric"):
        xbuf, xv = view(X0); ybuf, yv = view(Y)
        before = be.to_numpy(xbuf).copy()
        sm.apply_dev(direction, v, xv, yv, omega=1.1, num_iter=2)
        after = be.to_numpy(xbuf)
        got = after[:case.ncols, pad:pad + nv] if layout.endswith("right") else after[:nv, pad:pad + case.ncols].T
        outside = np.ones(after.shape, dtype=bool)
        if layout.endswith("right"): outside[:case.ncols, pad:pad + nv] = False
        else: outside[:nv, pad:pad + case.ncols] = False
        assert np.array_equal(np.isnan(after[outside]), np.isnan(before[outside])) and np.isnan(after[outside]).all()
        assert np.isfinite(got).all()
        for col in range(nv):
            x1 = sm.apply(direction, values, X0[:, col], Y[:, col], dtype, omega=1.1, num_iter=2)
            assert np.array_equal(got[:, col], x1), (layout, direction, col)
    sm.close()
def check_convergence(kk, be, case):
    values, _, _ = case.rounded
    xstar = np.random.default_rng(5).uniform(-1, 1, case.ncols)
    y = np.zeros(case.n)
    np.add.at(y, case.rows, values * xstar[case.entries])
    sm = Smoother(kk, be, case)
    for dtype in (np.float64, np.float32):
        e0 = np.linalg.norm(xstar)
        e2 = np.linalg.norm(sm.apply("symmetric", values, np.zeros(case.ncols), y, dtype, init_zero_x=True, num_iter=2) - xstar)
        e4 = np.linalg.norm(sm.apply("symmetric", values, np.zeros(case.ncols), y, dtype, init_zero_x=True, num_iter=4) - xstar)
        print("%r %s: error %.3g -> %.3g -> %.3g" % (case, np.dtype(dtype).name, e0, e2, e4))
        assert e2 < e0 and e4 < e2
    sm.close()
def check_statuses(kk, be, case):
    cap = kk._capi
    values, x0, y = case.rounded
    i32 = lambda a: be.from_numpy(np.array(a, dtype=np.int32))
    f64 = lambda a: be.from_numpy(np.array(a, dtype=np.float64))
    rm, ent, v, x, yd = i32(case.row_map), i32(case.entries), f64(values), f64(x0), f64(y)
    kh = kk.KokkosKernelsHandle(be)
    with pytest.raises(RuntimeError):
        kh.create_gs_handle("GS_NONSENSE")
    with pytest.raises(ValueError):                          # no GS handle on the KernelHandle
        kk.gauss_seidel_symbolic(kh, case.n, case.ncols, rm, ent)
    for algo in ("GS_CLUSTER", "GS_TWOSTAGE"):
        st, msg = status_of(kk, lambda: kh.create_gs_handle(algo))
        assert st == cap.ERR_UNSUPPORTED and algo in msg
    kh.create_gs_handle("GS_DEFAULT")
    gh = kh.get_gs_handle()
    apply_args = (case.n, case.ncols, rm, ent, v, x, yd)
    # apply, numeric and export before symbolic
    with pytest.raises(ValueError, match="symbolic"):
        kk.forward_sweep_gauss_seidel_apply(kh, *apply_args)
    with pytest.raises(ValueError, match="symbolic"):
        kk.gauss_seidel_numeric(kh, case.n, case.ncols, rm, ent, v)
    assert be.lib.kkamd_gs_apply(gh.h, case.n, case.ncols, be.ptr(rm), be.ptr(ent), be.ptr(v), be.ptr(x), 1, 0, be.ptr(yd), 1, 0, 1, 0, 1, 1.0, 1, 0, 0, 1,
                                 None) == cap.ERR_STATE
    st, msg = status_of(kk, lambda: gh.export("colors"))
    assert st == cap.ERR_STATE
    # num_cols < num_rows
    st, msg = status_of(kk, lambda: kk.gauss_seidel_symbolic(kh, case.n, case.n - 1, rm, ent))
    assert st == cap.ERR_INVALID_ARG and "num_cols" in msg
    # structural faults name the smallest offending row and the fault (rows 1 and 2 are faulty in the first two)
    for row_map, entries, word in (((0, 1, 2, 3), [0, 0, 1], "row 1: it has no diagonal"), ((0, 1, 4, 7), [0, 1, 0, 1, 2, 2, 1], "row 1: it has more than one"),
                                   ((0, 2, 4, 6), [0, 1, 1, 3, 2, 0], "row 1: a column is outside"), ((0, 2, 1, 3), [0, 1, 1], "not ascending")):
        st, msg = status_of(kk, lambda: kk.gauss_seidel_symbolic(kh, 3, 3, i32(row_map), i32(entries)))
        assert st == cap.ERR_INVALID_ARG and word in msg, msg
        assert not gh.is_symbolic_complete()
    # a good analysis; update_y = False on a first apply, and after num_vecs changed
    kk.gauss_seidel_symbolic(kh, case.n, case.ncols, rm, ent)
    assert gh.is_symbolic_complete() and not gh.is_numeric_called()
    with pytest.raises(ValueError, match="update_y"):
        kk.forward_sweep_gauss_seidel_apply(kh, *apply_args, False, False)
    assert not gh.is_numeric_called()
    # apply without numeric runs numeric itself
    kk.forward_sweep_gauss_seidel_apply(kh, *apply_args)
    assert gh.is_numeric_called()
    first = be.to_numpy(x).copy()
    kk.forward_sweep_gauss_seidel_apply(kh, case.n, case.ncols, rm, ent, v, x, None, False, False)   # the stored y
    x2 = be.from_numpy(np.zeros((case.ncols, 2))); y2 = be.from_numpy(np.zeros((case.n, 2)))
    with pytest.raises(ValueError, match="update_y"):
        kk.forward_sweep_gauss_seidel_apply(kh, case.n, case.ncols, rm, ent, v, x2, y2, False, False)
    # numeric repeated with -values: the inverse diagonal and the products both change sign, so a sweep from x0 with -y gives the same x;
    # with the same y it does not
    kk.gauss_seidel_numeric(kh, case.n, case.ncols, rm, ent, f64(-values))
    xa = f64(x0); kk.forward_sweep_gauss_seidel_apply(kh, case.n, case.ncols, rm, ent, f64(-values), xa, f64(-y))
    assert np.array_equal(be.to_numpy(xa), first)
    xb = f64(x0); kk.forward_sweep_gauss_seidel_apply(kh, case.n, case.ncols, rm, ent, f64(-values), xb, yd)
    assert not np.array_equal(be.to_numpy(xb), first)
    # a given inverse diagonal replaces the computed one: twice the inverse is omega = 2
    diag = np.zeros(case.n); diag[case.rows[case.rows == case.entries]] = values[case.rows == case.entries]
    kk.gauss_seidel_numeric(kh, case.n, case.ncols, rm, ent, v, f64(2.0 / diag))
    xc = f64(x0); kk.forward_sweep_gauss_seidel_apply(kh, *apply_args[:5], xc, yd)
    kk.gauss_seidel_numeric(kh, case.n, case.ncols, rm, ent, v, True)
    xd = f64(x0); kk.forward_sweep_gauss_seidel_apply(kh, *apply_args[:5], xd, yd, False, True, 2.0)
    assert np.allclose(be.to_numpy(xc), be.to_numpy(xd), rtol=1e-12, atol=0)
    # wrong sizes and types at numeric / apply, knob ranges, unknown keys
    assert be.lib.kkamd_gs_numeric(gh.h, case.n + 1, case.ncols, be.ptr(rm), be.ptr(ent), be.ptr(v), None, 0, 1, None) == cap.ERR_INVALID_ARG
    assert be.lib.kkamd_gs_numeric(gh.h, case.n, case.ncols, be.ptr(rm), be.ptr(ent), be.ptr(v), None, 0, 5, None) == cap.ERR_UNSUPPORTED
    for key, bad in (("lanes_per_row", 3), ("lanes_per_row", 128), ("lanes_per_row", -1), ("chain_rows", -1), ("chain_levels", 0),
                     ("long_row_threshold", -1), ("nonsense", 1)):
        st, msg = status_of(kk, lambda: gh.set(key, bad))
        assert st == cap.ERR_INVALID_ARG
    st, msg = status_of(kk, lambda: gh.get("nonsense"))
    assert st == cap.ERR_INVALID_ARG
    st, msg = status_of(kk, lambda: gh.export("nonsense"))
    assert st == cap.ERR_INVALID_ARG
    buf = np.zeros(2, dtype=np.int32)
    assert be.lib.kkamd_gs_export(gh.h, b"colors", buf.ctypes.data, 2) == cap.ERR_INVALID_ARG
    # plan_bytes stays inside the bound the header gives
    nnz = case.entries.shape[0]
    assert 0 < gh.get("plan_bytes") <= 48 * case.n + 12 * nnz + 8 * 1 * (case.n + case.ncols) + 16
    kh.destroy_gs_handle()
    assert kh.get_gs_handle() is None
def check_empty(kk, be, small):
    case = cases(small)["h0"][0]
    sm = Smoother(kk, be, case)
    check_coloring(sm)
    assert {k: sm.gh.get(k) for k in ("num_colors", "launches", "coloring_rounds", "long_rows")} == {"num_colors": 0, "launches": 0, "coloring_rounds": 0, "long_rows": 0}
    assert np.array_equal(sm.gh.export("color_xadj"), [0]) and sm.gh.export("colors").shape == (0,)
    x = sm.apply("symmetric", np.zeros(0), np.zeros(0), np.zeros(0), np.float64)
    assert x.shape == (0,)
    sm.close()


def check_supplied_colours(kk, be, small):
    cap = kk._capi
    case = cases(small)["b-rb"][1]
    sm = Smoother(kk, be, case)
    assert np.array_equal(sm.gh.export("colors"), case.supplied)
    # row 40 with the colour of row 41 has the colour of row 39 too: 39 is the smallest row with a neighbour of its colour
    for change, value, row, word in ((17, 0, 17, "outside"), (40, None, 39, "adjacent")):
        bad = case.supplied.copy()
        bad[change] = bad[change + 1] if value is None else value
        bad[150] = bad[151]                                 # a later offender: the smallest row is named
        sm.supplied = be.from_numpy(bad)
        st, msg = status_of(kk, sm.symbolic)
        assert st == cap.ERR_INVALID_ARG and "row %d:" % row in msg and word in msg, msg
        assert not sm.gh.is_symbolic_complete()
    sm.supplied = be.from_numpy(case.supplied)
    sm.symbolic()
    check_coloring(sm)
    sm.close()
    # case f: colours that are proper for A's rows as stored are still checked against the transposed graph
    case = cases(small)["f"][0]
    sm = Smoother(kk, be, case)
    sm.supplied = be.from_numpy(case.greedy[0])
    sm.symbolic()
    assert sm.gh.get("coloring_rounds") == 0 and np.array_equal(sm.gh.export("colors"), case.greedy[0])
    ptr, adj = case.adjacency
    v = int(np.flatnonzero(np.diff(ptr) > 0)[0])
    u = int(adj[ptr[v]:ptr[v + 1]].max())                   # row u > v stores (u, v); row v does not store (v, u)
    if u > v:
        bad = case.greedy[0].copy()
        bad[v] = bad[u]
        sm.supplied = be.from_numpy(bad)
        st, msg = status_of(kk, sm.symbolic)
        assert st == cap.ERR_INVALID_ARG and "row %d:" % min(u, v) in msg, msg
    sm.close()


def check_composition(kk, be, case):
    values, x0, y = case.rounded
    for dtype in (np.float64, np.float32):
        sm = Smoother(kk, be, case, threshold=64 if case.name == "e" else 0)
        v = be.from_numpy(values.astype(dtype)); yd = be.from_numpy(y.astype(dtype))
        new_x = lambda: be.from_numpy(x0.astype(dtype))
        # symmetric = forward, then backward on the stored y
        xs = new_x(); sm.apply_dev("symmetric", v, xs, yd, omega=1.25)
        xf = new_x(); sm.apply_dev("forward", v, xf, yd, omega=1.25); sm.apply_dev("backward", v, xf, None, update_y=False, omega=1.25)
        assert np.array_equal(be.to_numpy(xs), be.to_numpy(xf))
        # num_iter = 3 is three calls; two identical applies give identical bits
        for direction in ("forward", "backward", "symmetric"):
            x3 = new_x(); sm.apply_dev(direction, v, x3, yd, num_iter=3)
            x1 = new_x()
            for _ in range(3):
                sm.apply_dev(direction, v, x1, yd)
            assert np.array_equal(be.to_numpy(x3), be.to_numpy(x1))
            again = new_x(); sm.apply_dev(direction, v, again, yd, num_iter=3)
            assert np.array_equal(be.to_numpy(x3), be.to_numpy(again))
        # init_zero_x is a zero-filled x (ghost entries included)
        xz = be.from_numpy(np.full(case.ncols, np.nan, dtype=dtype)); sm.apply_dev("forward", v, xz, yd, init_zero_x=True)
        x0z = be.from_numpy(np.zeros(case.ncols, dtype=dtype)); sm.apply_dev("forward", v, x0z, yd)
        assert np.array_equal(be.to_numpy(xz), be.to_numpy(x0z))
        sm.close()


def check_ghost_entries(kk, be, small):
    for case in cases(small)["g"]:
        sm = Smoother(kk, be, case)
        for dtype in (np.float64, np.float32):
            check_exact(sm, dtype, "forward", 0.5)        # the ghost columns carry non-zero x0 into y
            values, x0, y = case.rounded
            x = sm.apply("symmetric", values, x0, y, dtype, num_iter=2)
            assert np.array_equal(x[case.n:], x0.astype(dtype)[case.n:])
            moved = x0.copy(); moved[case.n:] += 1.0
            x2 = sm.apply("symmetric", values, moved, y, dtype, num_iter=2)
            assert not np.array_equal(x2[:case.n], x[:case.n])
        sm.close()

