"""Row-partitioned SpMV (csrc/kk_dist.hip, dist.DistSpmv) on the CPU, exactly: the C implementation compiled for the SIMT emulator, the collectives through
dist._GlooTransport, every rank a process.  What runs and what is compared is in dist_cases.py: signed integer matrices (band, band-odd, scattered,
dense-col, blockdiag) cut by ragged partitions, by partitions with an empty first, middle or last rank and by a shard shorter than the band; the five
(offsets, A.values, vectors) triples; three calls per operator with x and y0 drawn anew.  Every partial sum is an integer below 2^24
(test_case_shapes asserts the bound on the data), so any order of summation gives the same bits in float32 and float64 and every comparison is
`==` -- on values, and on bits where NaN is expected.  No tolerance.

Beyond the values: the operator's whole x buffer is seeded with a sentinel NaN pattern before every apply and read back as integers, so a halo entry
that did not arrive, arrived from the wrong offset of a peer's list, or was written where nothing belongs shows by itself (check 2); Inf, -0.0 and a
NaN payload cross the exchange as bits (3); exchange-then-SpMV equals the whole step (4); an x kept in the operator's window equals a foreign one (5);
parts / interior_rows follow a numpy restatement of dist_setup's rule (6) and sends / recvs the peers that share something (7).

Coverage pairing (dist_cases.plan; fixed, checked by dist_cases.check_plan in test_case_shapes): one mp.spawn per world, all of that world's operators
in the worker, a barrier between operators.  Every (case, partition) meets every mode of auto, halo, halo_set, allgather, allgather_collective; pair
number i with mode number j takes the type triple (i + j) mod 5 and runs without overlap when (i + j) mod 4 == 0: every triple meets every mode, every
mode runs with and without overlap.  World 2: 5 cases x 5 partitions x 5 modes = 125 operators (the equal cut is the one whose all-gathers go through the transport's collective), plus allgather_p2p once, which every rank must refuse
with ERR_UNSUPPORTED (mapped device memory between processes does not exist under the emulator) without anybody left waiting; world 3: 75; world 4:
25.  n = 300.

window_codes_min_knnz is set to 0 as in test_dist_gloo.py: the slab plans and the interior / boundary views then take the 16-bit column codes at
this size too, which is what the product's slabs run, instead of the plain tiles every small matrix would get.

Run time on the machine this was written on (no GPU, `-m "not gpu"`, the emulator library built): this module 47 s; test_dist_gloo.py 84 s.  (Both were measured with the entry-scanning kernels of dist_setup launched over no more workgroups than the slab has entries for; with 1024
workgroups whatever the slab, creating one operator took 4 to 5 s under the emulator, test_dist_gloo.py 196 s and this module's world 4 alone 123 s.)"""
import os
import sys
from datetime import timedelta

import numpy as np
import pytest

import dist_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _operators(world):
    ops = [op + (None,) for op in dc.plan(world, dc.N_SMALL)]
    if world == 2:
        ops.append(("band", "ragged", dict(dc.partitions(dc.N_SMALL, 2))["ragged"], dc.TYPES[0], "allgather_p2p", True, "ERR_UNSUPPORTED"))
    return ops


def _worker(rank, world, port, ret, progress):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import kk_loader
    from emu import emu_backend
    kk = kk_loader.load()
    from kokkos_kernels_amd.dist import DistSpmv
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=300))
    be = emu_backend.backend()
    kk._capi.check(be.lib, be.lib.kkamd_set_default(b"window_codes_min_knnz", 0))

    def make_op(A, offs, rank_, mode, overlap, vdt):
        return DistSpmv(A, offs, rank_, exchange=mode, overlap=overlap, dtype=vdt)

    fails, seen = [], []
    ops = _operators(world)
    for i, (case, pname, offs, types, mode, overlap, refuse) in enumerate(ops):
        progress[rank] = "operator %d of %d: %s %s %s %s overlap %s" % (i, len(ops), case, pname, dc.type_name(types), mode, overlap)
        fails += dc.check_rank(kk, be, make_op, rank, world, case, pname, types, mode, overlap, n=dc.N_SMALL,
                               expect_status=getattr(kk._capi, refuse) if refuse else None, between=dist.barrier, seen=seen)
        ret[rank] = {"fails": fails, "seen": seen}
        if any(f["check"] == -1 for f in fails):           # an exception: this rank is out of step with its peers
            return
    progress[rank] = "done"
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3, 4])
def test_row_partitioned_spmv_values(world):
    port = 20500 + 4 * (os.getpid() % 700) + world
    ret, problem, _ = dc.run_ranks(_worker, world, (port,), deadline=900)
    fails = [f for r in sorted(ret) for f in ret[r]["fails"]]
    for f in fails:
        print(f)
    assert problem is None, problem
    assert sorted(ret) == list(range(world)), sorted(ret)
    assert not fails, "%d failure records, first: %s" % (len(fails), fails[0])
    # every operator of the table was created on every rank (the one refusal of world 2 creates none), and the splits the cases are for happened
    seen = [ret[r]["seen"] for r in range(world)]
    assert all(len(s) == len(dc.plan(world, dc.N_SMALL)) for s in seen), [len(s) for s in seen]
    flat = [op for s in seen for op in s]
    assert {"halo", "halo_set", "allgather"} == {ex for ex, _, _, _, _ in flat}
    assert any(parts == 3 and rows > 0 and tiles > 0 and mod4 == 0 for _, parts, rows, tiles, mod4 in flat)
    assert any(parts == 0 for _, parts, _, _, _ in flat)
    if world < 4:
        assert any(parts == 3 and mod4 == 1 for _, parts, _, _, mod4 in flat)


def test_case_shapes():
    """what the cases are meant to reach, on the generated data alone (no library): the pairing's coverage, the exactness bound, `auto`'s choice from the
    two fractions, unequal wants between three ranks, the splits of band and band-odd, both directions of blockdiag"""
    for n in (dc.N_SMALL, dc.N_GPU):
        for world in (2, 3) + ((4,) if n == dc.N_SMALL else ()):
            dc.check_plan(dc.plan(world, n), dc.MODES)
            parts = dict(dc.partitions(n, world))
            for pname, offs in parts.items():
                assert offs[0] == 0 and offs[-1] == n and all(b >= a for a, b in zip(offs, offs[1:]))
                for case in dc.CASES:
                    A = dc.matrix(case, n, offs)
                    assert A.entries.dtype == np.int32 and A.row_map.dtype == np.int64
                    assert np.array_equal(A.values, np.rint(A.values)) and np.abs(A.values).min() >= 1 and np.abs(A.values).max() <= 4
                    assert (A.values < 0).any() and (A.values > 0).any()
                    assert dc.exactness_bound(A) < 2 ** 24, (case, pname)
            ragged = parts.get("ragged") or parts["two-narrow"]
            M = {c: dc.matrix(c, n, ragged) for c in dc.CASES}
            # auto: the range halo for the bands, the set halo for scattered columns, the all-gather when the set is most of the vector
            assert [dc.expected_auto(M[c], ragged) for c in dc.CASES] == ["halo", "halo", "halo_set", "allgather", "halo"]
            fr = [dc.fractions(M["scattered"], ragged, r) for r in range(world)]
            assert max(f for f, _ in fr) >= 0.5 > max(s for _, s in fr)
            fr = [dc.fractions(M["dense-col"], ragged, r) for r in range(world)]
            assert max(s for _, s in fr) >= 0.5
            # band: some rank splits into interior, head and tail; the interior starts on a row whose first entry is a multiple of 4
            sp = [dc.expected_split(M["band"], ragged, r, "halo", True) for r in range(world)]
            assert any(p == 3 and rows > 0 and M["band"].slab(ragged[r], ragged[r + 1])[0][lo] % 4 == 0 for r, (p, rows, (lo, _)) in enumerate(sp)), sp
            assert all(dc.expected_split(M["band"], ragged, r, "halo", False)[:2] == (1 if ragged[r + 1] > ragged[r] else 0, 0) for r in range(world))
            # band-odd: local row r >= 1 of a slab starts at entry 4 r + 1, so the walk never finds a multiple of 4 and stops 64 rows in.  A rank
            # with neighbours on both sides loses 66 rows at either end; what is left is at least m / 2 only for m >= 264: under the emulator
            # (n = 300) the ragged cuts do not split and the split with misaligned views comes from the long shard of `short`; at the GPU's size
            # every rank of the ragged cuts that owns a later slab splits, and its views start on misaligned entries
            for pname in ("ragged", "short") if world < 4 else ("two-narrow",):
                offs = parts[pname]
                A = dc.matrix("band-odd", n, offs)
                for r in range(world):
                    m = offs[r + 1] - offs[r]
                    rm = A.slab(offs[r], offs[r + 1])[0]
                    assert m == 0 or (np.diff(rm)[1:] == 4).all() and (m < 2 or rm[1] == 5) and (rm[1:] % 4 == 1).all()
                    p, rows, (lo, hi) = dc.expected_split(A, offs, r, "halo", True)
                    first_owner = not any(offs[q + 1] > offs[q] for q in range(r))
                    if m < 264 and not (first_owner and m >= 132):
                        assert (p, rows) == (1 if m else 0, 0), (n, world, pname, r, p, rows)
                    elif not first_owner:
                        assert p == 3 and lo == 66 and rm[lo] % 4 == 1 and rm[hi] % 4 == 1 and rows >= m // 2, (n, world, pname, r, p, rows, lo, hi)
                    else:
                        assert p == 2 and lo == 0 and rm[hi] % 4 == 1, (n, world, pname, r, p, rows, lo, hi)
            misaligned = [(pn, r) for pn, offs in parts.items() for r in range(world) if dc.expected_split(dc.matrix("band-odd", n, offs), offs, r, "halo", True)[2][0] == 66]
            assert misaligned or world == 4, (n, world)             # (world 4, n = 300: only rank 0 splits, with a misaligned tail)
            if n == dc.N_GPU:
                assert ("ragged", 1) in misaligned
            # blockdiag: the last owner imports nothing and is imported from; with three owners the first neither imports nor is imported from
            for kind in ("halo", "halo_set"):
                ex = [dc.expected_exchange(M["blockdiag"], ragged, r, kind)[:3] for r in range(world)]
                owners = [r for r in range(world) if ragged[r + 1] > ragged[r]]
                assert ex[owners[-1]][2] == 0 and ex[owners[-1]][1] == 1 and ex[owners[-2]][2] == 1, ex
                if len(owners) >= 3:
                    assert ex[owners[0]][1:] == (0, 0), ex
            if world == 3:
                # scattered columns between three ranks: what r wants from p is not what p wants from r, nor what r wants from its other peer
                offs = parts["ragged"]
                want = np.zeros((3, 3), dtype=np.int64)
                for r in range(3):
                    off = dc.slab_columns(M["scattered"], offs, r)[0]
                    for p in range(3):
                        want[r, p] = ((off >= offs[p]) & (off < offs[p + 1])).sum()
                assert all(want[r, p] != want[p, r] for r in range(3) for p in range(r)), want
                assert sum(len({int(v) for p, v in enumerate(want[r]) if p != r}) == 2 for r in range(3)) >= 2, want
                assert (want + np.eye(3, dtype=np.int64) > 0).all()
    # the two operators most likely to differ between the emulator and the GPU are in the GPU's world-2 run: band-odd through a halo with overlap (the
    # misaligned views) and a float32 split of band
    gpu2 = dc.plan(2, dc.N_GPU, dc.MODES + ("allgather_p2p",))
    dc.check_plan(gpu2, dc.MODES + ("allgather_p2p",))
    assert any(c == "band-odd" and pn == "ragged" and m in ("halo", "halo_set", "auto") and ov for c, pn, _, _, m, ov in gpu2)
    assert any(c == "band" and pn == "ragged" and m in ("halo", "halo_set", "auto") and ov and t[2] == np.float32 for c, pn, _, t, m, ov in gpu2)
