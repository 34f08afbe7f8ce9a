"""Cases and checks shared by tests/test_emu_mis2.py (emulator) and tests/test_gpu_mis2.py (GPU): the distance-2 maximal independent
set, the MIS-2 aggregation and the explicit coarsening.

The first half restates the reference's loops in numpy, one vectorised step per round, with the places they come from
(graph/impl/KokkosGraph_Distance2MIS_impl.hpp, common/src/KokkosKernels_SimpleUtils.hpp).  The library must give these results exactly:
the reference takes its priorities from a fixed hash of (vertex, round) and its ids from scans, so there is no tolerance anywhere.
The second half holds the graphs and the checks."""
import ctypes as C

import numpy as np

IN_SET, OUT_SET = np.uint32(0), np.uint32(0xFFFFFFFF)
LANES = (0, 1, 2, 4, 8, 16, 32, 64)          # 0 = the rule, then every width the knob takes


# the restatement --------------------------------------------------------------------------------------------------------------------

def xorshift_hash(v):
    """xorshiftHash<uint32_t> (KokkosKernels_SimpleUtils.hpp:377-385): v into 64 bits, x ^= x >> 12, x ^= x << 25, x ^= x >> 27,
    then the low 32 bits of (x * 2685821657736338717 - 1) >> 16, all modulo 2^64"""
    x = np.asarray(v).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(12))
    x = x ^ (x << np.uint64(25))
    x = x ^ (x >> np.uint64(27))
    with np.errstate(over="ignore"):
        y = x * np.uint64(2685821657736338717) - np.uint64(1)
    return ((y >> np.uint64(16)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def hash_by_hand(v):
    """the same formula in Python integers, for the pinned values"""
    x = v & 0xFFFFFFFF
    x ^= x >> 12
    x = (x ^ (x << 25)) & (2**64 - 1)
    x ^= x >> 27
    return (((x * 2685821657736338717 - 1) % 2**64) >> 16) & 0xFFFFFFFF


class Graph:
    """a CRS graph: n vertices, row_map (int64), entries (int32); columns >= n are ghosts"""

    def __init__(self, name, n, row_map, entries):
        self.name, self.n = name, int(n)
        self.row_map = np.asarray(row_map, dtype=np.int64)
        self.entries = np.asarray(entries, dtype=np.int32)
        self.deg = np.diff(self.row_map)
        self.rows = np.repeat(np.arange(self.n, dtype=np.int64), self.deg)
        self.ok = self.entries < self.n                      # "nei < nv" of every functor
        self.safe = np.where(self.ok, self.entries, 0).astype(np.int64)
        self.starts = self.row_map[:-1][self.deg > 0]
        self.nonempty = np.nonzero(self.deg > 0)[0]
        self._memo = {}

    def __repr__(self):
        return "%s(n=%d,nnz=%d)" % (self.name, self.n, self.entries.size)

    @property
    def nnz(self): return int(self.entries.size)

    def reduce_rows(self, ufunc, per_entry, self_value):
        """ufunc over {i} and the entries of row i"""
        out = np.array(self_value, copy=True)
        if self.entries.size:
            out[self.nonempty] = ufunc(out[self.nonempty], ufunc.reduceat(per_entry, self.starts))
        return out

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]


def nv_bits(n):
    """Distance2MIS_impl.hpp:57-62: the bit length of numVerts + 1"""
    return int(n + 1).bit_length()


def fast_status(g, verts, rnd):
    """RefreshRowStatus (:80-90)"""
    pr = xorshift_hash(xorshift_hash(verts.astype(np.uint32)) ^ xorshift_hash(np.uint32(rnd)))
    nb = nv_bits(g.n)
    hi = (pr.astype(np.uint64) << np.uint64(nb)) & np.uint64(0xFFFFFFFF) if nb < 32 else np.zeros(verts.size, np.uint64)
    s = ((verts.astype(np.uint64) + np.uint64(1)) | hi).astype(np.uint32)
    return np.where(s == OUT_SET, s - np.uint32(1), s)


def quality_status(g):
    """InitRowStatus (:533-546), in fp32 as the reference writes it; equal degrees: score 0 (the reference divides by zero)"""
    nb = nv_bits(g.n)
    deg_bits = 32 - nb
    v = np.arange(g.n, dtype=np.uint64) + np.uint64(1)
    if deg_bits <= 0:
        return v.astype(np.uint32)
    max_range = np.float32(np.uint32((1 << deg_bits) - 2))
    lo, hi = int(g.deg.min()), int(g.deg.max())
    if hi > lo:
        inv = np.float32(1.0) / np.float32(hi - lo)
        score = (g.deg - lo).astype(np.float32) * inv
    else:
        score = np.zeros(g.n, np.float32)
    scaled = (score * max_range).astype(np.int64).astype(np.uint64)
    return ((v + ((scaled << np.uint64(nb)) & np.uint64(0xFFFFFFFF))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


class Stall(Exception):
    """a round decided no row: the graph is not symmetric (the reference would not return)"""


def d2_mis(g, algo="MIS2_FAST", mask=None):
    """D2_MIS_RandomPriority::compute() (:312-381), compute(mask) (:385-458) and D2_MIS_FixedPriority::compute() (:746-775).  Every
    column is refreshed in every round: an OUT_SET column stays OUT_SET (a neighbour row is IN_SET for good, or all are OUT_SET for
    good), so this gives the statuses of the work lists and of the bitset.  Returns (set ascending, rounds)."""
    n = g.n
    if n == 0:
        return np.zeros(0, np.int32), 0
    quality = algo == "MIS2_QUALITY"
    undecided = np.ones(n, bool) if mask is None else (mask < 0)
    row = np.full(n, OUT_SET, np.uint32)
    if quality:
        row[undecided] = quality_status(g)[undecided]
    rounds = 0
    while undecided.any():
        if not quality:
            idx = np.nonzero(undecided)[0]
            row[idx] = fast_status(g, idx, rounds)
        # RefreshColStatus (:109-125)
        col = g.reduce_rows(np.minimum, np.where(g.ok, row[g.safe], OUT_SET), row)
        col[col == IN_SET] = OUT_SET
        # DecideSetFunctor (:178-209): OUT_SET when a column is, IN_SET when every column carries the row's status
        cmax = g.reduce_rows(np.maximum, np.where(g.ok, col[g.safe], IN_SET), col)
        cmin = g.reduce_rows(np.minimum, np.where(g.ok, col[g.safe], OUT_SET), col)
        out = undecided & (cmax == OUT_SET)
        into = undecided & ~out & (cmax == row) & (cmin == row)
        if not (out | into).any():
            raise Stall(rounds + 1)
        row[out] = OUT_SET
        row[into] = IN_SET
        undecided &= ~(out | into)
        rounds += 1
    return np.nonzero(row == IN_SET)[0].astype(np.int32), rounds


class Aggregation:
    """D2_MIS_Aggregation::compute (:1088-1106)"""

    def __init__(self, g, secondary):
        n = g.n
        labels = np.full(n, -1, np.int32)
        roots = np.zeros(n, bool)
        e64 = g.safe
        # phase 1 (:820-852)
        m1, self.rounds = d2_mis(g)
        roots[m1] = True
        agg_of = np.full(n, -1, np.int32)
        agg_of[m1] = np.arange(m1.size, dtype=np.int32)
        labels[m1] = agg_of[m1]
        sel = roots[g.rows] & g.ok
        labels[e64[sel]] = agg_of[g.rows[sel]]
        self.primary = num = int(m1.size)
        # phase 2 (:854-946)
        self.masked_rounds = self.secondary = 0
        if secondary:
            m2, self.masked_rounds = d2_mis(g, mask=labels)
            free = g.ok & (g.safe != g.rows) & (labels[e64] == -1)
            size = 1 + np.bincount(g.rows[free], minlength=n)
            chosen = m2[size[m2] >= 3]
            ids = np.full(n, -1, np.int32)
            ids[chosen] = num + np.arange(chosen.size, dtype=np.int32)
            sel = free & (ids[g.rows] >= 0)
            labels[chosen] = ids[chosen]
            roots[chosen] = True
            labels[e64[sel]] = ids[g.rows[sel]]
            self.secondary = int(chosen.size)
            num += self.secondary
        self.num = num
        self.unlabelled = int((labels == -1).sum())
        # phase 3 (:948-1084), from the frozen labels
        old = labels.copy()
        sizes = np.bincount(old[old >= 0], minlength=max(num, 1)).astype(np.int64)
        same = g.ok & (g.safe != g.rows) & (old[e64] == old[g.rows]) & (old[g.rows] != -1)
        connect = np.bincount(g.rows[same], minlength=n).astype(np.int64)
        t_agg = np.zeros((n, 8), np.int64); t_con = np.zeros((n, 8), np.int64); t_root = np.zeros((n, 8), bool)
        tracked = np.zeros(n, np.int64)
        walking = ~roots
        self.ninth = np.zeros(n, bool)
        slot = np.arange(8)
        for k in range(int(g.deg.max()) if n else 0):          # the k-th stored entry of every row at once
            i = np.nonzero(walking & (g.deg > k))[0]
            p = g.row_map[i] + k
            j = g.safe[p]
            keep = g.ok[p] & (j != i)
            na = old[j]
            keep &= (na != -1) & (na != old[i])
            i, j, na = i[keep], j[keep], na[keep]
            eq = (t_agg[i] == na[:, None]) & (slot[None, :] < tracked[i][:, None])
            have = eq.any(axis=1)
            at = np.where(have, eq.argmax(axis=1), tracked[i])
            full = ~have & (tracked[i] == 8)                     # the ninth aggregate: break (:1028-1031)
            self.ninth[i[full]] = True
            walking[i[full]] = False
            i, j, na, at, have = i[~full], j[~full], na[~full], at[~full], have[~full]
            t_agg[i[~have], at[~have]] = na[~have]
            tracked[i[~have]] += 1
            t_root[i, at] |= roots[j]
            t_con[i, at] += 1
        best_root = (old >= 0).astype(np.int64)
        best_agg = old.astype(np.int64)
        best_con = connect.copy()
        best_size = np.where(old >= 0, sizes[np.maximum(old, 0)], 0)
        for k in range(8):
            live = (tracked > k) & ~roots
            s = sizes[t_agg[:, k]]
            r = t_root[:, k].astype(np.int64)
            better = live & ((r > best_root) | ((r == best_root) & ((t_con[:, k] > best_con) | ((t_con[:, k] == best_con) & (s < best_size)))))
            best_root = np.where(better, r, best_root); best_con = np.where(better, t_con[:, k], best_con)
            best_size = np.where(better, s, best_size); best_agg = np.where(better, t_agg[:, k], best_agg)
        self.labels = best_agg.astype(np.int32)


def coarse_pairs(g, labels):
    """the (coarse row, coarse column) of every cross-cluster entry, in the library's uncompressed order: the vertices of a cluster
    ascending, their entries in stored order"""
    order = np.argsort(labels, kind="stable")
    lens = g.deg[order]
    idx = np.repeat(g.row_map[order] - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()), dtype=np.int64)
    r, c = labels[g.rows[idx]], labels[g.safe[idx]]
    keep = g.ok[idx] & (r != c)
    return r[keep], c[keep], order


def coarse_graph(g, labels, nc, compress):
    r, c, order = coarse_pairs(g, labels)
    if compress:
        pairs = np.unique(np.stack([r, c], axis=1), axis=0) if r.size else np.zeros((0, 2), np.int32)
        r, c = pairs[:, 0], pairs[:, 1]
    rm = np.zeros(nc + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=nc), out=rm[1:])
    inv_off = np.zeros(nc + 1, np.int32)
    np.cumsum(np.bincount(labels, minlength=nc), out=inv_off[1:])
    return rm, c.astype(np.int32), inv_off, order.astype(np.int32)


# graphs -----------------------------------------------------------------------------------------------------------------------------

def from_edges(name, n, u, v):
    """symmetric graph of the undirected edges (u, v)"""
    a = np.concatenate([u, v]).astype(np.int64); b = np.concatenate([v, u]).astype(np.int64)
    order = np.lexsort((b, a))
    a, b = a[order], b[order]
    rm = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(a, minlength=n), out=rm[1:])
    return Graph(name, n, rm, b)


def lattice(name, dims, full):
    """7-point (or 5-point) stencil, or with full=True the 27-point (9-point) one, diagonal stored"""
    dims = tuple(dims)
    n = int(np.prod(dims))
    coords = np.stack(np.unravel_index(np.arange(n), dims), axis=1)
    offs = np.stack(np.meshgrid(*[[-1, 0, 1]] * len(dims), indexing="ij"), axis=-1).reshape(-1, len(dims))
    if not full:
        offs = offs[np.abs(offs).sum(axis=1) <= 1]
    rows, cols = [], []
    for o in offs:
        c = coords + o
        ok = ((c >= 0) & (c < np.array(dims))).all(axis=1)
        rows.append(np.nonzero(ok)[0]); cols.append(np.ravel_multi_index(c[ok].T, dims))
    a, b = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((b, a))
    rm = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(a, minlength=n), out=rm[1:])
    return Graph(name, n, rm, b[order])


def random_graph(name, n, half_degree, seed, shuffle=True):
    rng = np.random.default_rng(seed)
    u = np.repeat(np.arange(n), half_degree); v = rng.integers(0, n, u.size)
    keep = u != v
    pairs = np.unique(np.stack([np.minimum(u, v)[keep], np.maximum(u, v)[keep]], axis=1), axis=0)
    g = from_edges(name, n, pairs[:, 0], pairs[:, 1])
    if not shuffle:
        return g
    ent = g.entries.copy()
    for i in range(n):                                         # stored order matters to phase 3
        rng.shuffle(ent[g.row_map[i]:g.row_map[i + 1]])
    return Graph(name, n, g.row_map, ent)


def path(name, n):
    return from_edges(name, n, np.arange(n - 1), np.arange(1, n))


def ghosts_and_isolated():
    """a 9 x 9 5-point lattice whose vertices 10 k are cut off (isolated), and a ghost column >= n in every third row"""
    g = lattice("x", (9, 9), False)
    cut = np.zeros(g.n, bool); cut[::10] = True
    keep = ~cut[g.rows] & ~cut[g.safe] & (g.rows != g.safe)
    rows, ent = g.rows[keep], g.entries[keep]
    gr = np.arange(0, g.n, 3); gr = gr[~cut[gr]]
    rows = np.concatenate([rows, gr]); ent = np.concatenate([ent, g.n + (gr % 7).astype(np.int32)])
    order = np.argsort(rows, kind="stable")
    rm = np.zeros(g.n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=g.n), out=rm[1:])
    return Graph("ghosts", g.n, rm, ent[order])


def self_loops():
    """a random graph with the diagonal stored in every second row, twice in every sixth"""
    g = random_graph("x", 300, 3, 5)
    rows = np.concatenate([g.rows, np.arange(0, 300, 2), np.arange(0, 300, 6)])
    ent = np.concatenate([g.entries, np.arange(0, 300, 2), np.arange(0, 300, 6)])
    order = np.argsort(rows, kind="stable")
    rm = np.zeros(301, np.int64)
    np.cumsum(np.bincount(rows, minlength=300), out=rm[1:])
    return Graph("selfloops", 300, rm, ent[order])


def ring(name, n, reach):
    """every vertex adjacent to the `reach` next and previous ones: regular, all degrees equal"""
    u = np.repeat(np.arange(n), reach); v = (u + np.tile(np.arange(1, reach + 1), n)) % n
    return from_edges(name, n, u, v)


def hub(n, spokes):
    """a path with vertex 0 adjacent to `spokes` more vertices: one row longer than 64 entries"""
    far = np.arange(2, 2 + spokes) * ((n - 1) // (spokes + 2))
    far = np.unique(far[far > 1])
    return from_edges("hub", n, np.concatenate([np.arange(n - 1), np.zeros(far.size, np.int64)]), np.concatenate([np.arange(1, n), far]))


def directed_cycle():
    """0 -> 1 -> 2 -> 0: no row sees its own status in the next column, so no round decides anything"""
    return Graph("stall", 3, [0, 1, 2, 3], [1, 2, 0])


def cases(small):
    """small: emulator sizes.  Otherwise the sizes that cross the boundaries of the compaction on the GPU: more than one workgroup,
    more than 2,048 workgroup counts in one scan (the 2-D lattice: 2 * 409,600 / 256 = 3,200 counts at one lane per vertex), the
    4,000-vertex random graph, the 27-point 40^3 lattice"""
    c = {
        "lat7": lattice("lat7", (12, 12, 12), False),
        "lat27": lattice("lat27", (12, 12, 12), True),
        "rand": random_graph("rand", 4000, 6, 11),
        "path": path("path", 200 if small else 700),
        "ghosts": ghosts_and_isolated(),
        "selfloops": self_loops(),
        "ring": ring("ring", 500, 3),
        "hub": hub(400 if small else 1500, 90),
    }
    if not small:
        c["lat5big"] = lattice("lat5big", (640, 640), False)
        c["lat27big"] = lattice("lat27big", (40, 40, 40), True)
    return c


_CASES = {}


def all_cases(small, names=None):
    if small not in _CASES:
        _CASES[small] = cases(small)
    return [g for k, g in _CASES[small].items() if names is None or k in names]


def reference(g, what):
    """the restatement's result, computed once per graph and left unchanged"""
    if what in ("MIS2_FAST", "MIS2_QUALITY"):
        return g.memo(what, lambda: d2_mis(g, what))
    return g.memo(what, lambda: Aggregation(g, what == "aggregate"))


# checks -----------------------------------------------------------------------------------------------------------------------------

class Device:
    """a graph in the backend's memory"""

    def __init__(self, kk, be, g, offset_dtype=np.int32):
        self.kk, self.be, self.g = kk, be, g
        self.rm = be.from_numpy(g.row_map.astype(offset_dtype))
        self.ent = be.from_numpy(g.entries if g.nnz else np.zeros(1, np.int32))
        if not g.nnz:
            self.ent = self.ent[:0]

    def mis(self, algo):
        st = {}
        out = self.kk.graph_d2_mis(self.rm, self.ent, algo, backend=self.be, stats=st)
        return np.array(self.be.to_numpy(out), copy=True), st

    def labels(self, secondary):
        st = {}
        fn = self.kk.graph_mis2_aggregate if secondary else self.kk.graph_mis2_coarsen
        lab, num = fn(self.rm, self.ent, backend=self.be, stats=st)
        return np.array(self.be.to_numpy(lab), copy=True), num, st

    def coarsen(self, labels, nc, compress, inverse_map=True):
        out = self.kk.graph_explicit_coarsen(self.rm, self.ent, self.be.from_numpy(np.asarray(labels, np.int32)), nc, compress, inverse_map, backend=self.be)
        return [np.array(self.be.to_numpy(a), copy=True) for a in out]


def set_lanes(be, lanes):
    rc = be.lib.kkamd_set_default(b"mis2_lanes_per_vertex", int(lanes))
    assert rc == 0, be.lib.kkamd_last_error()


def closed_cover(g, member):
    """for every vertex the number of members in its closed neighbourhood, duplicates and self-loops counted once"""
    keep = g.ok & (g.safe != g.rows)
    pairs = np.unique(np.stack([g.rows[keep], g.safe[keep]], axis=1), axis=0) if keep.any() else np.zeros((0, 2), np.int64)
    cover = member.astype(np.int64)
    return cover + np.bincount(pairs[:, 0], weights=member[pairs[:, 1]], minlength=g.n).astype(np.int64), pairs


def check_independent_and_maximal(g, mis):
    """from the definition: no two members within distance 2 (no vertex has two members in its closed neighbourhood), and every vertex has
    a member within distance 2 (some vertex of its closed neighbourhood has one in its own)"""
    member = np.zeros(g.n, bool); member[mis] = True
    assert member.sum() == mis.size and (np.diff(mis) > 0).all()
    cover, pairs = closed_cover(g, member)
    assert cover.max() <= 1, "two members within distance 2"
    near = cover > 0
    reach = near.astype(np.int64) + np.bincount(pairs[:, 0], weights=near[pairs[:, 1]], minlength=g.n).astype(np.int64)
    assert (reach > 0).all(), "a vertex with no member within distance 2: not maximal"


ALGOS = ("MIS2_FAST", "MIS2_QUALITY")


def check_mis(kk, be, g, offset_dtype=np.int32, algos=ALGOS):
    d = Device(kk, be, g, offset_dtype)
    for algo in algos:
        exp, rounds = reference(g, algo)
        got, st = d.mis(algo)
        assert np.array_equal(got, exp), (g, algo)
        assert st["rounds"] == rounds and st["masked_rounds"] == 0
        assert st["host_syncs"] == 2 + rounds                # kkamd.h: one per round plus two per call
        assert st["scratch_bytes"] > 0 and st["launches"] >= 4 * rounds
        check_independent_and_maximal(g, got)
        again, st2 = d.mis(algo)
        assert np.array_equal(again, got) and st2 == st


def check_aggregation(kk, be, g, offset_dtype=np.int32):
    d = Device(kk, be, g, offset_dtype)
    for secondary in (False, True):
        exp = reference(g, "aggregate" if secondary else "coarsen")
        lab, num, st = d.labels(secondary)
        assert num == exp.num and np.array_equal(lab, exp.labels), (g, secondary)
        assert (st["rounds"], st["masked_rounds"]) == (exp.rounds, exp.masked_rounds)
        assert (st["primary_aggregates"], st["secondary_aggregates"], st["unlabelled_before_phase3"]) == (exp.primary, exp.secondary, exp.unlabelled)
        assert st["host_syncs"] == (3 + exp.rounds + exp.masked_rounds if secondary else 2 + exp.rounds)
        assert lab.min() >= 0 and lab.max() < num             # a symmetric graph: every vertex labelled
        lab2, num2, st2 = d.labels(secondary)
        assert num2 == num and np.array_equal(lab2, lab) and st2 == st


def check_lanes(kk, be, g, quality=True, lanes_values=LANES):
    """no output depends on the lanes per vertex"""
    d = Device(kk, be, g)
    try:
        base = None
        for lanes in lanes_values:
            set_lanes(be, lanes)
            mf, sf = d.mis("MIS2_FAST"); mq, sq = d.mis("MIS2_QUALITY" if quality else "MIS2_FAST")
            lab, num, sa = d.labels(True)
            crm, cent, ioff, ilab = d.coarsen(lab, num, False)
            got = (mf, mq, lab, crm, cent, ioff, ilab)
            rounds = (sf["rounds"], sq["rounds"], sa["rounds"], sa["masked_rounds"], num)
            if base is None:
                base = (got, rounds)
            assert rounds == base[1] and all(np.array_equal(a, b) for a, b in zip(got, base[0])), lanes
    finally:
        set_lanes(be, 0)
    assert be.lib.kkamd_set_default(b"mis2_lanes_per_vertex", 3) == kk._capi.ERR_INVALID_ARG
    assert be.lib.kkamd_set_default(b"mis2_lanes_per_vertex", 128) == kk._capi.ERR_INVALID_ARG


def check_coarsening(kk, be, g, offset_dtype=np.int32):
    d = Device(kk, be, g, offset_dtype)
    agg = reference(g, "aggregate")
    rng = np.random.default_rng(3)
    for labels, nc in ((agg.labels, agg.num), (rng.integers(0, 7, g.n).astype(np.int32), 9)):    # 9: two clusters without a vertex
        for compress in (True, False):
            rm, ent, inv_off, order = coarse_graph(g, labels, nc, compress)
            crm, cent, ioff, ilab = d.coarsen(labels, nc, compress)
            assert crm.dtype == np.dtype(offset_dtype)
            assert np.array_equal(crm, rm) and np.array_equal(cent, ent), (g, compress)
            assert np.array_equal(ioff, inv_off) and np.array_equal(ilab, order)
            assert cent.size <= g.nnz
            if compress:                                     # the set definition: sorted, no duplicate, no diagonal
                for c in range(nc):
                    row = cent[crm[c]:crm[c + 1]]
                    assert (np.diff(row) > 0).all() and c not in row
        two = d.coarsen(labels, nc, True, inverse_map=False)
        assert len(two) == 2 and np.array_equal(two[0], coarse_graph(g, labels, nc, True)[0])


def _status(kk, fn):
    try:
        fn()
    except kk.KkamdError as e:
        return e.status, str(e)
    raise AssertionError("no error raised")


def check_statuses(kk, be, g):
    """every error status of kkamd.h's section"""
    lib, INV = be.lib, kk._capi.ERR_INVALID_ARG
    d = Device(kk, be, g)
    # a row map that does not ascend, a negative entry: the smallest offending row
    rm = g.row_map.astype(np.int32).copy(); rm[5], rm[6] = rm[6], rm[5]
    bad = Device(kk, be, g); bad.rm = be.from_numpy(rm)
    first = 4 if g.deg[4] and rm[5] < rm[4] else 5
    for fn in (lambda: bad.mis("MIS2_FAST"), lambda: bad.labels(True), lambda: bad.coarsen(np.zeros(g.n, np.int32), 1, True)):
        st, msg = _status(kk, fn)
        assert st == INV and "row_map" in msg and "row %d:" % first in msg, msg
    ent = g.entries.copy(); ent[g.row_map[9]] = -1; ent[g.row_map[20]] = -3
    bad = Device(kk, be, g); bad.ent = be.from_numpy(ent)
    for fn in (lambda: bad.mis("MIS2_QUALITY"), lambda: bad.labels(False)):
        st, msg = _status(kk, fn)
        assert st == INV and "row 9:" in msg, msg
    # the stall
    s = Device(kk, be, directed_cycle())
    for fn in (lambda: s.mis("MIS2_FAST"), lambda: s.mis("MIS2_QUALITY"), lambda: s.labels(False), lambda: s.labels(True)):
        st, msg = _status(kk, fn)
        assert st == INV and "graph is not symmetric" in msg, msg
    for algo in ("MIS2_FAST", "MIS2_QUALITY"):
        try:
            d2_mis(directed_cycle(), algo)
            raise AssertionError("the restatement decided a row")
        except Stall:
            pass
    # algorithm, offset type, sizes
    cnt = C.c_int64(); nnz = C.c_int64(7)
    assert lib.kkamd_graph_d2_mis(g.n, be.ptr(d.rm), 0, be.ptr(d.ent), 2, be.ptr(d.ent), C.byref(cnt), None, be.stream()) == INV
    assert b"graph_d2_mis: invalid algorithm" in lib.kkamd_last_error()
    assert lib.kkamd_graph_d2_mis(g.n, be.ptr(d.rm), 5, be.ptr(d.ent), 1, be.ptr(d.ent), C.byref(cnt), None, be.stream()) == INV
    assert lib.kkamd_graph_mis2_aggregate(-1, be.ptr(d.rm), 0, be.ptr(d.ent), 1, be.ptr(d.ent), C.byref(cnt), None, be.stream()) == INV
    assert lib.kkamd_graph_mis2_aggregate(g.n, None, 0, be.ptr(d.ent), 1, be.ptr(d.ent), C.byref(cnt), None, be.stream()) == INV
    # labels outside [0, num_coarse): the smallest offending vertex
    labels = reference(g, "aggregate").labels.copy()
    nc = reference(g, "aggregate").num
    lab = labels.copy(); lab[17] = nc; lab[40] = -1
    st, msg = _status(kk, lambda: d.coarsen(lab, nc, True))
    assert st == INV and "vertex 17:" in msg, msg
    # a capacity that is too small: the true count, nothing written
    for compress in (1, 0):
        rm, ent, _, _ = coarse_graph(g, labels, nc, bool(compress))
        crm = be.from_numpy(np.full(nc + 1, -7, np.int32)); cent = be.from_numpy(np.full(ent.size, -7, np.int32))
        dl = be.from_numpy(labels)
        args = (g.n, be.ptr(d.rm), 0, be.ptr(d.ent), be.ptr(dl), nc, compress, be.ptr(crm), be.ptr(cent))
        assert lib.kkamd_graph_explicit_coarsen(*args, ent.size - 1, C.byref(nnz), None, None, be.stream()) == INV
        assert b"capacity" in lib.kkamd_last_error() and nnz.value == ent.size
        assert (be.to_numpy(crm) == -7).all() and (be.to_numpy(cent) == -7).all()
        assert lib.kkamd_graph_explicit_coarsen(*args, ent.size, C.byref(nnz), None, None, be.stream()) == 0
        assert np.array_equal(be.to_numpy(crm), rm) and np.array_equal(be.to_numpy(cent), ent)
    assert lib.kkamd_graph_explicit_coarsen(g.n, be.ptr(d.rm), 0, be.ptr(d.ent), be.ptr(d.ent), nc, 1, be.ptr(d.rm), None, -1, C.byref(nnz), None, None,
                                            be.stream()) == INV


def check_empty(kk, be):
    for dt in (np.int32, np.int64):
        rm = be.from_numpy(np.zeros(1, dt)); ent = be.from_numpy(np.zeros(1, np.int32))[:0]
        for algo in ("MIS2_FAST", "MIS2_QUALITY"):
            st = {}
            assert kk.graph_d2_mis(rm, ent, algo, backend=be, stats=st).shape[0] == 0
            assert st["launches"] == 0 and st["host_syncs"] == 0
        for fn in (kk.graph_mis2_coarsen, kk.graph_mis2_aggregate):
            st = {}
            lab, num = fn(rm, ent, backend=be, stats=st)
            assert lab.shape[0] == 0 and num == 0 and st["launches"] == 0
        crm, cent, ioff, ilab = kk.graph_explicit_coarsen(rm, ent, ent, 0, True, True, backend=be)
        assert np.array_equal(be.to_numpy(crm), [0]) and cent.shape[0] == 0 and np.array_equal(be.to_numpy(ioff), [0]) and ilab.shape[0] == 0
    with_rows = kk.graph_explicit_coarsen(rm, ent, ent, 3, False, backend=be)
    assert np.array_equal(be.to_numpy(with_rows[0]), [0, 0, 0, 0])


def check_shapes(small):
    """the cases reach the paths they are meant for; all from the restatement"""
    c = _CASES.setdefault(small, cases(small))
    for k in (0, 1, 5, 0xFFFFFFFF):
        assert int(xorshift_hash(np.uint32(k))) == hash_by_hand(k)
    # by hand: x = 0 stays 0, 0 * c - 1 = 2^64 - 1, >> 16 leaves 48 ones, the low 32 are all ones;
    # x = 1: 1 ^ (1 << 25) = 0x2000001, >> 27 adds nothing, 0x2000001 * 2685821657736338717 - 1 = 0x47e4ce4b896cdd1c modulo 2^64, bits 16..47 of which are 0xce4b896c
    assert hash_by_hand(0) == 0xFFFFFFFF and hash_by_hand(1) == 0xce4b896c and hash_by_hand(5) == 0x12e85fb3
    a7, a27 = reference(c["lat7"], "aggregate"), reference(c["lat27"], "aggregate")
    assert (a7.rounds, a7.primary, a7.secondary, a7.unlabelled) == (8, 179, 73, 325)
    assert (a27.rounds, a27.primary, a27.secondary) == (7, 50, 42)
    ar = reference(c["rand"], "aggregate")
    assert int(ar.ninth.sum()) == 658                        # the walk stops at the ninth neighbouring aggregate; pins the generator too
    assert reference(c["path"], "aggregate").secondary == 0 and reference(c["path"], "aggregate").unlabelled > 0
    gh = c["ghosts"]
    assert (gh.deg == 0).sum() >= 9 and (gh.entries >= gh.n).sum() > 10
    assert np.isin(np.nonzero(gh.deg == 0)[0], reference(gh, "MIS2_FAST")[0]).all()     # an isolated vertex is its own root
    sl = c["selfloops"]
    assert (sl.entries == sl.rows).sum() > 150
    assert c["ring"].deg.min() == c["ring"].deg.max() == 6    # MIS2_QUALITY's equal-degree rule
    assert c["hub"].deg.max() > 64
    q = quality_status(c["hub"])
    assert len(set(q.tolist())) == c["hub"].n and q.min() > 0 and q.max() < 0xFFFFFFFF
    if not small:
        assert 2 * -(-c["lat5big"].n // 256) > 2048            # the scan of the workgroup counts recurses
        assert c["lat27big"].n == 64000
