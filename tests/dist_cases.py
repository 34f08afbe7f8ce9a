"""Generated inputs and the per-rank checks of the row-partitioned SpMV value tests (CPU only; shared by test_emu_dist_values.py, which runs
the C implementation under the SIMT emulator over gloo, and test_gpu_dist_values.py, which runs it between processes on one GPU).

Matrices (global n x n, row_map int64, entries int32, values integers with 1 <= |a| <= 4 and a random sign; numpy.random.default_rng with seeds
derived from the case; n = 300 under the emulator, 4000 on the GPU).  Two of them depend on the partition they are cut by:
  band       rows reference r-2 .. r+2, clipped to the matrix; rows with r % 10 == 9 are empty.  Middle rows of a shard reference only the shard's
             own columns: the interior / boundary split happens.
  band-odd   every row holds exactly 4 entries, its four nearest columns without the diagonal, and the FIRST row of every rank's slab holds its
             diagonal as well.  Local row r >= 1 of a slab then starts at entry 4 r + 1: no row start but the slab's first is a multiple of 4, the
             64-step alignment walk of dist_setup gives up, and the part views begin on misaligned entries and values.
  scattered  the structure of test_dist_gloo._scattered_matrix: the band, plus two columns from anywhere in every tenth row.  The column range
             of a slab is everything, the column set small: `auto` takes the column-set halo, and with three ranks every rank wants another
             count from every peer.
  dense-col  the band, plus FAR_PER_ROW columns from anywhere in every third row.  (One such column per row, which is what comes to mind first,
             reaches a share of 1 - exp(-m / (3 n)) < 0.2 of the off-slab columns whatever the cut; the set halo has to move at least half of
             them before `auto` gives it up, which eight columns per row do: 1 - exp(-8 m / (3 n)) = 0.59 at m = n / 3.)  `auto` takes the all-gather.
  blockdiag  the band with the slab of the LAST rank that owns rows cut down to its own columns: that rank imports nothing (recvs == 0) while its
             neighbour still imports from it.  With three or more ranks that own rows the FIRST of them is cut off both ways: it imports
             nothing and nobody imports from it (sends == recvs == 0), and it still joins every collective.

Partitions (row offsets; a = n // 2 - 7):
  world 2    ragged [0, n // 3 + 5, n]; empty-first [0, 0, n]; empty-last [0, n, n]; short [0, 3, n] -- a shard shorter than the band; equal
             [0, n // 2, n] -- the only cut with equal shards, so the only one whose all-gather goes through the transport's collective, in place
             (allgather_form 0; every other cut sends every shard to every peer point to point, form 1)
  world 3    ragged [0, n // 4 + 3, 2 n // 3 + 1, n]; empty-middle [0, a, a, n]; short [0, 3, n - 1, n]
  world 4    [0, a, a + 1, a + 1, n] (emulator only)

Exact values.  x and y0 are integers in [-8, 8], drawn anew for every call from a generator every rank seeds alike; (alpha, beta) is (2, -1),
(1, 0) with y seeded with NaN, and (-1, 1).  |alpha| sum |a x| + |beta y0| < 2^24 in every row (13 entries at most, |a x| <= 32; asserted by
exactness_bound), so every partial sum in every order is an integer that float32 holds: any kernel gives the same bits, in float32 and in float64,
and the comparison with the long-double sum of the products (expected) is `==`.  There is no tolerance anywhere in this module.

Types (TYPES): (offsets, A.values, vectors) = (int32, f64, f64), (int64, f32, f32), (int64, f64, f64), (int32, f32, f32), (int32, f32, f64).

check_rank runs one operator on one rank and returns failure records (it raises nothing: a rank that raised alone would leave its peers in a
collective).  Checks, by the number they carry in the records:
  1  values: y == expected over the three calls
  2  what the exchange wrote: the operator's whole x buffer is filled with a sentinel NaN bit pattern before every apply and read as unsigned
     integers afterwards.  Own shard and every off-slab column the slab references: x's bits.  Column-set halo: every other entry still the
     sentinel.  Column-range halo: every entry outside own + [cmin, cmax] still the sentinel.  All-gathers: every entry x's bits.  exchange_bytes
     == elem * (distinct off-slab columns | clipped range | n - m).
  3  specials travel as bits: +Inf, -Inf, -0.0 and a NaN with a payload in x, each at a column some rank imports and at a column its owner's slab
     references; the x buffer holds those bits (check 2 on this call), y is NaN exactly where the products say so and equal elsewhere (Inf included)
  4  apply(what=1) then apply(what=2) gives the bits of apply(what=0)
  5  an x kept in x_local() gives the bits a foreign shard gives (a rank without rows has no window; it still calls apply, which must return)
  6  parts and interior_rows equal expected_split, a restatement of dist_setup's rule, with overlap on and off
  7  sends and recvs equal the number of peers with a non-empty intersection (the all-gathers list every peer, an empty shard as an empty message)
  0  the exchange the operator reports: `auto` by expected_auto (the two fractions, the largest over the ranks decides); everything else as asked
"""
import ctypes as C
import functools
import traceback
import zlib

import numpy as np

N_SMALL, N_GPU = 300, 4000
FAR_PER_ROW = 8
CASES = ("band", "band-odd", "scattered", "dense-col", "blockdiag")
MODES = ("auto", "halo", "halo_set", "allgather", "allgather_collective")
TYPES = ((np.int32, np.float64, np.float64), (np.int64, np.float32, np.float32), (np.int64, np.float64, np.float64),
         (np.int32, np.float32, np.float32), (np.int32, np.float32, np.float64))
ALPHA_BETA = ((2.0, -1.0), (1.0, 0.0), (-1.0, 1.0))
_UINT = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}
# +Inf, -Inf, -0.0 and a quiet NaN with a payload (not the sentinel's), as bits
SPECIAL_BITS = {np.dtype(np.float64): (0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000, 0x7FF80000DEC0DE01),
                np.dtype(np.float32): (0x7F800000, 0xFF800000, 0x80000000, 0x7FC0DE01)}


def type_name(types):
    return "i%d/%s/%s" % (np.dtype(types[0]).itemsize * 8, np.dtype(types[1]).name, np.dtype(types[2]).name)


class Matrix:
    """one global CRS matrix (row_map int64, entries int32, values float64 holding small integers)"""

    def __init__(self, name, n, rows):
        self.name, self.n = name, n
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        self.row_map = np.zeros(n + 1, dtype=np.int64); np.cumsum(lens, out=self.row_map[1:])
        self.entries = np.array([c for r in rows for c in r], dtype=np.int32)
        rng = np.random.default_rng(zlib.crc32(name.encode()) + n)
        nnz = self.entries.size
        self.values = (rng.integers(1, 5, nnz) * rng.choice([-1, 1], nnz)).astype(np.float64)
        self.row_of = np.repeat(np.arange(n, dtype=np.int64), lens)

    def slab(self, r0, r1):
        """rows [r0, r1): (local row_map, entries with global columns, values)"""
        sl = slice(self.row_map[r0], self.row_map[r1])
        return self.row_map[r0:r1 + 1] - self.row_map[r0], self.entries[sl], self.values[sl]


def _band_rows(n):
    return [[] if r % 10 == 9 else list(range(max(0, r - 2), min(n - 1, r + 2) + 1)) for r in range(n)]


@functools.lru_cache(maxsize=None)
def matrix(case, n, offsets):
    """the case's matrix for the partition `offsets` (a tuple)"""
    rng = np.random.default_rng(zlib.crc32(case.encode()) + 7 * n)
    if case == "band":
        rows = _band_rows(n)
    elif case == "band-odd":
        rows = []
        for r in range(n):
            lo = min(max(r - 2, 0), n - 5)
            rows.append([c for c in range(lo, lo + 5) if c != r])
        for k in range(len(offsets) - 1):
            if offsets[k + 1] > offsets[k]:
                rows[offsets[k]] = sorted(rows[offsets[k]] + [offsets[k]])
    elif case == "scattered":
        rows = [sorted(set(range(max(0, r - 2), min(n - 1, r + 2) + 1)) | ({int(v) for v in rng.integers(0, n, size=2)} if r % 10 == 3 else set()))
                for r in range(n)]
    elif case == "dense-col":
        rows = [sorted(set(b) | ({int(v) for v in rng.integers(0, n, size=FAR_PER_ROW)} if r % 3 == 0 else set())) for r, b in enumerate(_band_rows(n))]
    elif case == "blockdiag":
        rows = _band_rows(n)
        owners = [k for k in range(len(offsets) - 1) if offsets[k + 1] > offsets[k]]
        if len(owners) >= 2:
            k = owners[-1]
            for r in range(offsets[k], offsets[k + 1]):
                rows[r] = [c for c in rows[r] if offsets[k] <= c < offsets[k + 1]]
        if len(owners) >= 3:
            j = owners[0]
            for r in range(n):
                mine = offsets[j] <= r < offsets[j + 1]
                rows[r] = [c for c in rows[r] if (offsets[j] <= c < offsets[j + 1]) == mine]
    else:
        raise KeyError(case)
    return Matrix(case, n, rows)


def partitions(n, world):
    a = n // 2 - 7
    if world == 2:
        return (("ragged", (0, n // 3 + 5, n)), ("empty-first", (0, 0, n)), ("empty-last", (0, n, n)), ("short", (0, 3, n)), ("equal", (0, n // 2, n)))
    if world == 3:
        return (("ragged", (0, n // 4 + 3, 2 * n // 3 + 1, n)), ("empty-middle", (0, a, a, n)), ("short", (0, 3, n - 1, n)))
    if world == 4:
        return (("two-narrow", (0, a, a + 1, a + 1, n)),)
    raise KeyError(world)


def plan(world, n, modes=MODES):
    """the fixed pairing: every (case, partition) of the world with every mode; the type triple and the overlap flag rotate with the position
    of the pair and of the mode, so that every triple meets every mode and every mode runs without overlap (asserted by check_plan).
    Returns [(case, partition name, offsets, types, mode, overlap)]"""
    out = []
    pairs = [(c, pn, offs) for c in CASES for pn, offs in partitions(n, world)]
    for i, (c, pn, offs) in enumerate(pairs):
        for j, mode in enumerate(modes):
            out.append((c, pn, offs, TYPES[(i + j) % len(TYPES)], mode, (i + j) % 4 != 0))
    return out


def check_plan(ops, modes):
    """the coverage the pairing promises, on the table alone"""
    pairs = {(c, pn) for c, pn, _, _, _, _ in ops}
    for mode in modes:
        assert {(c, pn) for c, pn, _, _, m, _ in ops if m == mode} == pairs, mode
        assert {type_name(t) for _, _, _, t, m, _ in ops if m == mode} == {type_name(t) for t in TYPES}, mode
        assert any(not ov for _, _, _, _, m, ov in ops if m == mode) and any(ov for _, _, _, _, m, ov in ops if m == mode), mode


# ------------------------------------------------------------------------------------------- the reference, by definition
def expected(A, x, alpha, beta, y0):
    """(y, S): y = alpha A x + beta y0 as long-double sums of the expanded products (y0 is not read for beta == 0), S = sum |a x| per row"""
    ld = np.longdouble
    assert np.finfo(ld).nmant > np.finfo(np.float64).nmant, "np.longdouble is no wider than float64 here"
    with np.errstate(all="ignore"):
        prod = A.values.astype(ld) * np.asarray(x, dtype=ld)[A.entries]
        s = np.zeros(A.n, dtype=ld); np.add.at(s, A.row_of, prod)
        S = np.zeros(A.n, dtype=ld); np.add.at(S, A.row_of, np.abs(prod))
        y = ld(alpha) * s
        if beta != 0:
            y = y + ld(beta) * np.asarray(y0, dtype=ld)
    return y, S


def exactness_bound(A):
    """the largest |alpha| sum |a x| + |beta y0| any row can reach with |x|, |y0| <= 8 and the (alpha, beta) of ALPHA_BETA"""
    S = np.zeros(A.n); np.add.at(S, A.row_of, np.abs(A.values) * 8.0)
    return float(max(abs(a) * (S.max() if A.n else 0.0) + abs(b) * 8.0 for a, b in ALPHA_BETA))


# ------------------------------------------------------------------------------------------- what the operator must report
def slab_columns(A, offsets, rank):
    """(distinct off-slab columns of the rank's slab, cmin, cmax) -- cmin, cmax = INT32_MAX, -1 for a slab without entries"""
    r0, r1 = offsets[rank], offsets[rank + 1]
    ent = A.slab(r0, r1)[1].astype(np.int64)
    off = np.unique(ent[(ent < r0) | (ent >= r1)])
    return off, (int(ent.min()) if ent.size else 2 ** 31 - 1), (int(ent.max()) if ent.size else -1)


def range_piece(offsets, cmin, cmax, p):
    """the piece of [cmin, cmax] that rank p owns, as (lo, hi), empty when hi <= lo"""
    return max(cmin, offsets[p]), min(cmax + 1, offsets[p + 1])


def fractions(A, offsets, rank):
    """(range halo, set halo) as fractions of the all-gather's n - m entries (0 when the rank owns everything)"""
    world, n = len(offsets) - 1, offsets[-1]
    off, cmin, cmax = slab_columns(A, offsets, rank)
    full = n - (offsets[rank + 1] - offsets[rank])
    halo = sum(max(0, hi - lo) for lo, hi in (range_piece(offsets, cmin, cmax, p) for p in range(world) if p != rank))
    return (halo / full, off.size / full) if full > 0 else (0.0, 0.0)


def expected_auto(A, offsets):
    """`auto`: the range halo when it moves less than half of the all-gather on every rank, else the set halo when that does, else the all-gather"""
    fr = [fractions(A, offsets, r) for r in range(len(offsets) - 1)]
    frac, sfrac = max(f for f, _ in fr), max(s for _, s in fr)
    return "halo" if frac < 0.5 else ("halo_set" if sfrac < 0.5 else "allgather")


def expected_exchange(A, offsets, rank, kind):
    """kind: halo | halo_set | allgather.  (entries received, sends, recvs, must_x, must_sentinel) -- the two masks over the n columns"""
    world, n = len(offsets) - 1, offsets[-1]
    r0, r1 = offsets[rank], offsets[rank + 1]
    peers = [p for p in range(world) if p != rank]
    must_x = np.zeros(n, dtype=bool); must_x[r0:r1] = True
    off, cmin, cmax = slab_columns(A, offsets, rank)
    must_x[off] = True
    if kind == "allgather":
        return n - (r1 - r0), world - 1, world - 1, np.ones(n, dtype=bool), np.zeros(n, dtype=bool)
    if kind == "halo_set":
        recvs = sum(1 for p in peers if ((off >= offsets[p]) & (off < offsets[p + 1])).any())
        sends = 0
        for p in peers:
            poff = slab_columns(A, offsets, p)[0]
            sends += 1 if ((poff >= r0) & (poff < r1)).any() else 0
        return int(off.size), sends, recvs, must_x, ~must_x
    assert kind == "halo", kind
    keep = np.ones(n, dtype=bool); keep[r0:r1] = False
    count = recvs = sends = 0
    for p in peers:
        lo, hi = range_piece(offsets, cmin, cmax, p)
        if hi > lo:
            count += hi - lo; recvs += 1; keep[lo:hi] = False
        _, pmin, pmax = slab_columns(A, offsets, p)
        lo, hi = range_piece(offsets, pmin, pmax, rank)
        sends += 1 if hi > lo else 0
    return count, sends, recvs, must_x, keep


def expected_split(A, offsets, rank, kind, overlap):
    """(parts, interior_rows, (r_lo, r_hi)) by dist_setup's rule: the all-gathers never split; a halo operator with overlap takes the longest run
    of rows with only own columns (the first of equals), walks both ends inward at most 64 rows to a row start divisible by 4, drops the run
    when it is shorter than m / 2, and splits into interior, head and tail (empty ones left out) unless the run is the whole slab"""
    r0, r1 = offsets[rank], offsets[rank + 1]
    m = r1 - r0
    if m == 0:
        return 0, 0, (0, 0)
    if kind == "allgather":
        return 1, 0, (0, 0)
    rm, ent, _ = A.slab(r0, r1)
    lo = hi = 0
    if overlap and rm[-1] > 0:
        flag = np.zeros(m, dtype=bool)
        flag[np.repeat(np.arange(m), np.diff(rm))[(ent < r0) | (ent >= r1)]] = True
        best = run0 = 0
        for r in range(m + 1):
            if r == m or flag[r]:
                if r - run0 > best:
                    best, lo, hi = r - run0, run0, r
                run0 = r + 1
        k = 0
        while k < 64 and lo < hi and rm[lo] % 4 != 0:
            lo += 1; k += 1
        k = 0
        while k < 64 and hi > lo and rm[hi] % 4 != 0:
            hi -= 1; k += 1
        if hi - lo < m // 2:
            lo = hi = 0
    if hi > lo and not (lo == 0 and hi == m):
        return 1 + (1 if lo > 0 else 0) + (1 if hi < m else 0), hi - lo, (lo, hi)
    return 1, (m if (lo == 0 and hi == m) else 0), (lo, hi)


def special_columns(A, offsets):
    """eight columns for the four special values: four that some rank imports (fewer when fewer are imported, then reused) and four more that
    their owner's slab references"""
    world, n = len(offsets) - 1, offsets[-1]
    imported = np.unique(np.concatenate([slab_columns(A, offsets, r)[0] for r in range(world)] + [np.empty(0, np.int64)]))
    owner = lambda idx: np.searchsorted(np.asarray(offsets[1:]), idx, side="right")
    own_ref = np.unique(A.entries[owner(A.entries) == owner(A.row_of)]).astype(np.int64)
    imp = [int(imported[(i * max(imported.size // 4, 1)) % imported.size]) for i in range(4)] if imported.size else []
    rest = [int(c) for c in own_ref if int(c) not in imp]
    own = [rest[(1 + i * (len(rest) // 4)) % len(rest)] for i in range(4)]
    return imp, own


# ------------------------------------------------------------------------------------------- one operator on one rank
def _xbuf(be, op, n, vdt):
    """the operator's full-length x buffer as integers of the vectors' width (the second output of kkamd_dist_spmv_x_local): (fill, read)"""
    from kokkos_kernels_amd._capi import check
    p = C.c_void_p()
    check(be.lib, be.lib.kkamd_dist_spmv_x_local(op._op, None, C.byref(p)))
    u = _UINT[vdt]
    if be.name == "emu":
        v = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64 if vdt.itemsize == 8 else C.c_uint32)), shape=(n,))
        return (lambda bits: v.__setitem__(slice(None), bits)), (lambda: v.copy())
    import torch
    from kokkos_kernels_amd.dist import _DeviceView
    t = torch.as_tensor(_DeviceView(p.value, n, "<i8" if vdt.itemsize == 8 else "<i4"), device="cuda")
    return (lambda bits: t.fill_(int(bits))), (lambda: t.cpu().numpy().view(u).copy())


def check_rank(kk, be, make_op, rank, world, case, partition, types, mode, overlap, n=N_SMALL, expect_status=None, between=None, seen=None):
    """one operator of the plan on this rank: the checks of the module docstring.  make_op(A_local, offsets, rank, mode, overlap, vector dtype)
    creates the DistSpmv.  expect_status: the creation must be refused with this status (on every rank: nobody is left waiting).  between: the
    ranks' barrier, called after the last apply and before the operator is destroyed (not after a refused creation, which every rank meets).
    seen: a list that receives (exchange in use, parts, interior_rows, part0_tiles, first interior entry modulo 4) of every operator created.
    Returns a list of failure records; a record with check -1 is an exception, after which the rank should start nothing more."""
    fails = []
    who = {"rank": rank, "world": world, "case": case, "partition": partition, "types": type_name(types), "mode": mode, "overlap": overlap}

    def bad(check_no, detail):
        fails.append(dict(who, check=check_no, detail=detail))

    try:
        from parity_cases import SENTINEL_BITS
        offsets = dict(partitions(n, world))[partition]
        odt, adt, vdt = types[0], np.dtype(types[1]), np.dtype(types[2])
        u = _UINT[vdt]
        A0 = matrix(case, n, offsets)
        r0, r1 = offsets[rank], offsets[rank + 1]
        m = r1 - r0
        rm, ent, val = A0.slab(r0, r1)
        A = kk.CrsMatrix.from_host(m, n, rm, ent, val.astype(adt), offset_dtype=odt, backend=be)
        try:
            op = make_op(A, list(offsets), rank, mode, overlap, vdt)
        except kk.KkamdError as e:
            if expect_status is None or e.status != expect_status:
                bad(0, "creation refused with status %d: %s" % (e.status, e))
            return fails
        if expect_status is not None:
            bad(0, "creation was to be refused with status %d and succeeded" % expect_status)
            return fails
        # 0: the exchange in use
        kind = {"auto": expected_auto(A0, offsets), "halo": "halo", "halo_set": "halo_set"}.get(mode, "allgather")
        names = (kind,)
        if mode == "allgather_p2p":
            names = (mode,)
        elif kind == "allgather" and mode != "allgather_collective" and be.name != "emu":
            names = ("allgather", "allgather_p2p")       # on the GPU an operator that times its forms may keep the pulls of mapped memory
        if op.exchange_mode not in names:
            bad(0, "exchange %s, expected %s" % (op.exchange_mode, names))
        equal = len({b - a for a, b in zip(offsets, offsets[1:])}) == 1
        if mode == "allgather_collective" and op.allgather_form != (0 if equal else 1):      # the collective itself needs equal shards
            bad(0, "allgather_form %d with %s shards" % (op.allgather_form, "equal" if equal else "unequal"))
        count, sends, recvs, must_x, must_sent = expected_exchange(A0, offsets, rank, kind)
        if op.exchange_bytes != vdt.itemsize * count:
            bad(2, "exchange_bytes %d, expected %d * %d" % (op.exchange_bytes, vdt.itemsize, count))
        # 6, 7
        parts, interior, run = expected_split(A0, offsets, rank, kind, overlap)
        if (op.query("parts"), op.interior_rows) != (parts, interior):
            bad(6, "parts %d interior_rows %d, expected %d and %d (run %s)" % (op.query("parts"), op.interior_rows, parts, interior, run))
        if op.query("part0_rows") != (interior if parts > 1 else m):
            bad(6, "part0_rows %d" % op.query("part0_rows"))
        # the interior view has a plan of its own with tiles (which kernel a call then takes is decided at dispatch from the alignment of the view's
        # entries and values, and no query reports it)
        if parts > 1 and op.query("part0_tiles") <= 0:
            bad(6, "the interior view was not analysed: part0_tiles %d" % op.query("part0_tiles"))
        if (op.query("sends"), op.query("recvs")) != (sends, recvs):
            bad(7, "sends %d recvs %d, expected %d and %d" % (op.query("sends"), op.query("recvs"), sends, recvs))
        if seen is not None:
            seen.append((op.exchange_mode, op.query("parts"), op.interior_rows, op.query("part0_tiles"), int(rm[run[0]] % 4) if parts > 1 else 0))

        rng = np.random.default_rng(zlib.crc32(repr((case, partition, type_name(types), mode, overlap, world)).encode()))
        sentinel = SENTINEL_BITS[vdt]
        fill, read = _xbuf(be, op, n, vdt)
        sync = (lambda: None) if be.name == "emu" else __import__("torch").cuda.synchronize

        def draw():
            return rng.integers(-8, 9, n).astype(vdt), rng.integers(-8, 9, n).astype(vdt)

        def apply(alpha, x, beta, y0, what=(0,), xdev=None):
            """y of the rank's shard (NaN-seeded for beta == 0) after the given steps; x, y0 global"""
            yd = be.from_numpy(np.full(m, np.nan, dtype=vdt) if beta == 0 else y0[r0:r1].copy())
            xd = be.from_numpy(x[r0:r1].copy()) if xdev is None else xdev
            for w in what:
                op.apply(alpha, xd, beta, yd, what=w)
            sync()
            return be.to_numpy(yd)

        def check_buffer(check_no, x, tag):
            got, xb = read(), x.view(u)
            wrong = must_x & (got != xb)
            if wrong.any():
                c = int(np.flatnonzero(wrong)[0])
                bad(check_no, "%s: %d entries of the x buffer do not hold x, first column %d: %#x, x %#x" % (tag, int(wrong.sum()), c, int(got[c]), int(xb[c])))
            wrong = must_sent & (got != sentinel)
            if wrong.any():
                c = int(np.flatnonzero(wrong)[0])
                bad(check_no, "%s: %d entries outside the imported set were written, first column %d: %#x" % (tag, int(wrong.sum()), c, int(got[c])))

        # 1, 2: three calls, x and y0 new every time
        for alpha, beta in ALPHA_BETA:
            x, y0 = draw()
            fill(sentinel)
            got = apply(alpha, x, beta, y0)
            exp, S = expected(A0, x, alpha, beta, y0)
            assert abs(alpha) * float(S.max() if n else 0) + abs(beta) * 8 < 2 ** 24
            if not np.array_equal(got, exp[r0:r1].astype(vdt)):
                d = np.flatnonzero(got != exp[r0:r1].astype(vdt))
                bad(1, "alpha %g beta %g: %d rows differ, first local row %d: %r, expected %r" % (alpha, beta, d.size, int(d[0]), got[d[0]], float(exp[r0 + d[0]])))
            check_buffer(2, x, "alpha %g beta %g" % (alpha, beta))
        # 3: specials
        x, y0 = draw()
        imp, own = special_columns(A0, offsets)
        xu = x.view(u)
        for i, bits in enumerate(SPECIAL_BITS[vdt]):
            for cols in (imp, own):
                if cols:
                    xu[cols[i]] = bits
        fill(sentinel)
        got = apply(1.0, x, 0.0, y0)
        with np.errstate(all="ignore"):
            exp = expected(A0, x.astype(np.longdouble), 1.0, 0.0, y0)[0][r0:r1].astype(vdt)
        nan = np.isnan(exp)
        if not np.array_equal(np.isnan(got), nan) or not np.array_equal(got[~nan], exp[~nan]):
            d = np.flatnonzero((np.isnan(got) != nan) | (~nan & (got != exp)))
            bad(3, "%d rows differ with Inf / NaN / -0.0 in x, first local row %d: %r, expected %r" % (d.size, int(d[0]), got[d[0]], exp[d[0]]))
        check_buffer(3, x, "specials")
        # 4: exchange and SpMV as two steps
        # (the pair runs first, on a new x over a buffer full of sentinels: the exchange-only step has to bring everything the SpMV-only step reads,
        # and it must not touch y)
        x, y0 = draw()
        fill(sentinel)
        xd, yd = be.from_numpy(x[r0:r1].copy()), be.from_numpy(y0[r0:r1].copy())
        op.apply(2.0, xd, -1.0, yd, what=1)
        sync()
        check_buffer(4, x, "after what = 1")
        if not np.array_equal(be.to_numpy(yd).view(u), y0[r0:r1].view(u)):
            bad(4, "what = 1 wrote y")
        op.apply(2.0, xd, -1.0, yd, what=2)
        sync()
        steps = be.to_numpy(yd)
        fill(sentinel)
        whole = apply(2.0, x, -1.0, y0)
        if not np.array_equal(whole.view(u), steps.view(u)):
            bad(4, "what = 1, 2 differs from what = 0 in %d rows" % int((whole.view(u) != steps.view(u)).sum()))
        if not np.array_equal(whole, expected(A0, x, 2.0, -1.0, y0)[0][r0:r1].astype(vdt)):
            bad(4, "what = 0 differs from the expected values")
        # 5: x kept in the operator's own window, written there after the whole buffer was filled with sentinels; the foreign shard second
        x, y0 = draw()
        fill(sentinel)
        if m > 0:
            xl = op.x_local()
            if be.name == "emu":
                xl = xl.numpy(); xl[:] = x[r0:r1]
            else:
                xl.copy_(be.from_numpy(x[r0:r1].copy()))
            window = apply(-1.0, x, 1.0, y0, xdev=xl)
        else:
            window = apply(-1.0, x, 1.0, y0)
        check_buffer(5, x, "x in x_local()")
        fill(sentinel)
        foreign = apply(-1.0, x, 1.0, y0)
        if not np.array_equal(foreign.view(u), window.view(u)):
            bad(5, "x in x_local() differs from a foreign shard in %d rows" % int((foreign.view(u) != window.view(u)).sum()))
        if not np.array_equal(foreign, expected(A0, x, -1.0, 1.0, y0)[0][r0:r1].astype(vdt)):
            bad(5, "a foreign shard differs from the expected values")
        if between:
            between()                    # every rank is done with the operator before any rank frees its buffers
        del op
    except Exception as e:               # reported, never raised: the peers of a rank that raised alone would wait in a collective
        bad(-1, "%r\n%s" % (e, traceback.format_exc()))
    return fails


# ------------------------------------------------------------------------------------------- ranks as processes, with a deadline
def run_ranks(target, world, args, deadline):
    """starts `world` processes target(rank, world, *args, ret, progress), joins them until `deadline` seconds have passed and terminates what
    is still running then (20 s after a rank ended without reporting "done": its peers wait for it in a collective).  Returns (ret as a dict,
    problem, hard): problem is None, or says which rank ended by a signal, with a non-zero status or at the deadline, and what every rank reported
    last; hard is True when a rank ended by a signal or had to be terminated."""
    import time
    from multiprocessing import connection
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret, progress = mgr.dict(), mgr.dict()
        procs = [ctx.Process(target=target, args=(r, world) + tuple(args) + (ret, progress)) for r in range(world)]
        for p in procs:
            p.start()
        end = time.monotonic() + deadline
        while any(p.is_alive() for p in procs) and time.monotonic() < end:
            connection.wait([p.sentinel for p in procs if p.is_alive()], timeout=1.0)
            # a rank that ended without reporting "done" has left its peers in a collective: they get a moment to notice, not the whole deadline
            if any(not p.is_alive() and progress.get(r) != "done" for r, p in enumerate(procs)):
                end = min(end, time.monotonic() + 20)
        late = [r for r, p in enumerate(procs) if p.is_alive()]
        for p in procs:
            if p.is_alive():
                p.terminate()
        for p in procs:
            p.join(10)
            if p.is_alive():
                p.kill(); p.join()
        codes = [p.exitcode for p in procs]
        problem = None
        if late:
            problem = "ranks %s were still running after %d s and were terminated" % (late, deadline)
        elif any(c != 0 for c in codes):
            problem = "exit codes %s (negative: ended by that signal)" % codes
        if problem:
            problem += "; last reports: %s" % {r: progress.get(r) for r in range(world)}
        return dict(ret), problem, bool(late) or any(c is not None and c < 0 for c in codes)
