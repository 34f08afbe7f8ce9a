"""Row-partitioned SpMV (csrc/kk_dist.hip, dist.DistSpmv) on the GPU (`-m gpu`), exactly: the ranks are separate processes on the one GPU, each with its own
device buffers, the collectives staged through the host by dist._GlooDeviceTransport as in test_gpu_dist_two_process.py -- so the pack, scatter,
rebase, min / max and flag kernels, the communication stream with its events and the local SpMV on the part views run on the device at the types
and edges test_emu_dist_values.py runs under the emulator, through the same dist_cases.check_rank.

Cases, partitions, the exactness argument (every partial sum an integer below 2^24: `==` in float32 and float64, no tolerance) and the checks are in
dist_cases.py; the matrices have n = 4000 rows here.  The interior view of `band` then holds 1336 to 2653 rows and 6000 to 12000 entries, several tiles
of its own plan.  What the queries show, and check 6 asserts, is that the interior view was analysed: part0_rows == interior_rows and part0_tiles > 0.
They do not show which kernel a call takes: the dispatch uses a view's plan only when the view's entries start 8-byte aligned and its values 16-byte
(float32: 8-byte) aligned, which for a view of the slab means an even first entry, and no query reports that decision.  band's interior starts at a
multiple of 4 entries; band-odd's starts 66 rows into the slab at an entry that is 1 modulo 4, an odd one, so by that rule its plan is passed over:
asserted here is only that this split happens (first interior entry 1 modulo 4) and that its values are exact.

Coverage pairing (dist_cases.plan, fixed): every (case, partition) with every mode; pair i with mode j takes type triple (i + j) mod 5 and runs
without overlap when (i + j) mod 4 == 0.
  world 2  ragged, empty-first, empty-last, short, equal; auto, halo, halo_set, allgather, allgather_collective and allgather_p2p
           (HSA_ENABLE_IPC_MODE_LEGACY as the two-process test sets it): 150 operators.  band-odd through the halos with overlap and the float32 split of
           band are here, so they run first (test_emu_dist_values.test_case_shapes asserts that the table holds them).
  world 3  ragged, empty-middle, short; every mode but allgather_p2p: 75 operators.  That keeps the FORCED pulls of mapped memory out of three processes,
           not every mapping: `allgather`, and `auto` where it resolves to the all-gather (dense-col, the short cuts), are the exchange that times its forms
           at creation, and on the device that exchange offers every rank's x buffer to every peer (hipIpcGetMemHandle / hipIpcOpenMemHandle), times
           the pulls next to the other forms and may keep them -- check_rank accepts allgather_p2p as its result.  A rank whose mapping fails says so
           in a flag and the operator goes on without that form.  This has run between three processes on the MI355X and passed.
Five processes in all, three at a time at the most.

So that trouble ends the run: the process group has a timeout of 120 s, a rank stops at its first exception, the parent joins with a deadline, terminates
what is left and fails with what every rank reported last; and when the world-2 run ended by a signal or at its deadline the world-3 test does not
start."""
import os
import sys
from datetime import timedelta

import pytest

import dist_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
# why the two-process run did not end by itself, if it did not: the three-process test reads it.  A module global, so the guard holds when both tests run
# in one process in file order, which is how the suite runs them; a selection of the three-process test alone, or tests spread over processes, has no
# two-process run to look at and starts.
_WORLD2 = {"problem": None}


def _worker(rank, world, port, modes, ret, progress):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    import kk_loader
    kk = kk_loader.load()
    from kokkos_kernels_amd.dist import DistSpmv, _GlooDeviceTransport
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    progress[rank] = "joining the process group"
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    torch.cuda.set_device(0)
    be = kk.torch_backend()

    def make_op(A, offs, rank_, mode, overlap, vdt):
        return DistSpmv(A, offs, rank_, exchange=mode, overlap=overlap, dtype=vdt, transport=_GlooDeviceTransport(None, world))

    fails, seen = [], []
    ops = dc.plan(world, dc.N_GPU, modes)
    for i, (case, pname, offs, types, mode, overlap) in enumerate(ops):
        progress[rank] = "operator %d of %d: %s %s %s %s overlap %s" % (i, len(ops), case, pname, dc.type_name(types), mode, overlap)
        fails += dc.check_rank(kk, be, make_op, rank, world, case, pname, types, mode, overlap, n=dc.N_GPU, between=dist.barrier, seen=seen)
        ret[rank] = {"fails": fails, "seen": seen}
        if any(f["check"] == -1 for f in fails):           # an exception (a HIP error among them): nothing more is started on the device
            return
    progress[rank] = "done"
    dist.destroy_process_group()


def _run(world, modes):
    port = 24000 + 4 * (os.getpid() % 700) + world
    ret, problem, hard = dc.run_ranks(_worker, world, (port, modes), deadline=400)
    fails = [f for r in sorted(ret) for f in ret[r]["fails"]]
    for f in fails:
        print(f)
    if world == 2 and hard:
        _WORLD2["problem"] = problem
    assert problem is None, problem
    assert sorted(ret) == list(range(world)), sorted(ret)
    assert not fails, "%d failure records, first: %s" % (len(fails), fails[0])
    seen = [ret[r]["seen"] for r in range(world)]
    assert all(len(s) == len(dc.plan(world, dc.N_GPU, modes)) for s in seen), [len(s) for s in seen]
    return [op for s in seen for op in s]


def test_values_between_two_processes():
    seen = _run(2, dc.MODES + ("allgather_p2p",))
    # the paths this run is for were taken: the pulls of mapped memory, a split whose analysed interior view starts on an aligned entry, and a split
    # whose views start on misaligned entries
    assert any(ex == "allgather_p2p" for ex, _, _, _, _ in seen)
    assert any(ex in ("halo", "halo_set") and parts == 3 and rows > 0 and tiles > 0 and mod4 == 0 for ex, parts, rows, tiles, mod4 in seen)
    assert any(ex in ("halo", "halo_set") and parts == 3 and rows > 0 and mod4 == 1 for ex, parts, rows, tiles, mod4 in seen)


def test_values_between_three_processes():
    if _WORLD2["problem"] is not None:
        pytest.fail("not started: the two-process run did not end by itself (%s)" % _WORLD2["problem"])
    seen = _run(3, dc.MODES)
    assert {"halo", "halo_set", "allgather"} <= {ex for ex, _, _, _, _ in seen}
    assert any(parts == 3 and mod4 == 1 for _, parts, _, _, mod4 in seen) and any(parts == 0 for _, parts, _, _, _ in seen)
