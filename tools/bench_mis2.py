"""MIS-2 and MIS-2 aggregation: times of kk_mis2.hip against this library's own handle-less SpMV on the same matrix and against the other
graph analysis a multigrid setup pays, gauss_seidel_symbolic with computed colours, in the same process.  One JSON line per case on
stdout, appended to --out, stamped with the hash of kk_mis2.hip.

  python tools/bench_mis2.py [--cases 27pt_100,7pt_100,27pt_200,7pt_200,rmat_20] [--lanes 0] [--out profiles/mis2/bench_mis2.jsonl]

Graphs: the 27-point and 7-point stencils on n^3 points (diagonal stored, columns ascending, int32 offsets) and R-MAT (a, b, c =
0.57, 0.19, 0.19, 8 edges per vertex before symmetrising) of 2^scale vertices, symmetrised, duplicates merged, diagonal stored once.
Times: the median of 10 calls after 2 warm-up calls, a pair of events on the stream around each call (every call ends in a host
synchronisation of its own, so the event time is the call).  gauss_seidel_symbolic is the second of two calls on the host clock.
Byte model of the first round, when both work lists hold every vertex (later rounds are shorter; their lengths are not exported):
  2 n (4 + 2 * 4 + 4 + 4) + 2 (nnz + n) (4 + 4)     per list entry: the entry, two row offsets, the status written, the piece of tmp;
                                                   per entry of the closed neighbourhood: the column index and the gathered status"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import kk_loader  # noqa: E402

kk = kk_loader.load()


def event_median_ms(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def csr_from_pairs(n, r, c):
    """rows ascending, columns ascending inside a row, duplicates merged"""
    key = torch.unique(r.long() * n + c.long())
    r, c = (key // n), (key % n).int()
    rm = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    rm[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    assert int(rm[-1]) < 2**31
    return rm.int().contiguous(), c.contiguous()


def lattice(n, stencil):
    N = n * n * n
    i = torch.arange(N, dtype=torch.int64, device="cuda")
    x, y, z = i % n, (i // n) % n, i // (n * n)
    rows, cols = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if stencil == "7pt" and abs(dx) + abs(dy) + abs(dz) > 1:
                    continue
                ok = (x + dx >= 0) & (x + dx < n) & (y + dy >= 0) & (y + dy < n) & (z + dz >= 0) & (z + dz < n)
                rows.append(i[ok]); cols.append(i[ok] + dx + n * (dy + n * dz))
    return (N,) + csr_from_pairs(N, torch.cat(rows), torch.cat(cols))


def rmat(scale, edge_factor=8, seed=1):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    N, m = 1 << scale, edge_factor << scale
    r = torch.zeros(m, dtype=torch.int64, device="cuda"); c = torch.zeros(m, dtype=torch.int64, device="cuda")
    for _ in range(scale):
        u = torch.rand(m, device="cuda", generator=g)
        r = 2 * r + (u >= 0.76).long()                         # quadrants: [0, .57) 00, [.57, .76) 01, [.76, .95) 10, [.95, 1) 11
        c = 2 * c + (((u >= 0.57) & (u < 0.76)) | (u >= 0.95)).long()
    d = torch.arange(N, dtype=torch.int64, device="cuda")
    return (N,) + csr_from_pairs(N, torch.cat([r, c, d]), torch.cat([c, r, d]))


def run(name, lanes):
    kind, size = name.split("_")
    n, rm, ent = rmat(int(size)) if kind == "rmat" else lattice(int(size), kind)
    nnz = int(ent.shape[0])
    be = kk.torch_backend()
    assert be.lib.kkamd_set_default(b"mis2_lanes_per_vertex", lanes) == 0
    line = {"graph": name, "rows": n, "nnz": nnz, "offset": "int32", "lanes_per_vertex": lanes}
    for key, fn in (("mis2_fast", lambda st: kk.graph_d2_mis(rm, ent, "MIS2_FAST", stats=st)),
                    ("coarsen", lambda st: kk.graph_mis2_coarsen(rm, ent, stats=st)),
                    ("aggregate", lambda st: kk.graph_mis2_aggregate(rm, ent, stats=st))):
        st = {}
        ms = event_median_ms(lambda: fn(st))
        line[key + "_event_ms"] = round(ms, 4)
        line[key + "_stats"] = st
        rounds = st["rounds"] + st["masked_rounds"]
        line[key + "_ms_per_round"] = round(ms / max(rounds, 1), 4)
    labels, num = kk.graph_mis2_aggregate(rm, ent)
    line["num_aggregates"] = num
    line["explicit_coarsen_event_ms"] = round(event_median_ms(lambda: kk.graph_explicit_coarsen(rm, ent, labels, num, True), 5, 1), 4)
    A = kk.CrsMatrix(n, n, rm, ent, torch.ones(nnz, dtype=torch.float64, device="cuda"))
    x = torch.rand(n, dtype=torch.float64, device="cuda"); y = torch.zeros(n, dtype=torch.float64, device="cuda")
    line["spmv_event_ms"] = round(event_median_ms(lambda: kk.spmv("N", 1.0, A, x, 0.0, y), 20, 3), 4)
    line["aggregate_over_spmv"] = round(line["aggregate_event_ms"] / line["spmv_event_ms"], 2)
    model = 2 * n * 20 + 2 * (nnz + n) * 8
    line["model_bytes_first_round"] = model
    try:
        kh = kk.KokkosKernelsHandle(be)
        kh.create_gs_handle("GS_DEFAULT")
        kk.gauss_seidel_symbolic(kh, n, n, rm, ent, True, None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kk.gauss_seidel_symbolic(kh, n, n, rm, ent, True, None)
        torch.cuda.synchronize()
        line["gs_symbolic_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        line["gs_coloring_rounds"] = kh.get_gs_handle().get("coloring_rounds")
        line["aggregate_over_gs_symbolic"] = round(line["aggregate_event_ms"] / line["gs_symbolic_ms"], 3)
        kh.destroy_gs_handle()
    except kk.KkamdError as e:                                 # recorded, not hidden: the colouring's own limits are not this tool's subject
        line["gs_symbolic_ms"] = None
        line["gs_symbolic_error"] = str(e)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="27pt_100,7pt_100,27pt_200,7pt_200,rmat_20")
    ap.add_argument("--lanes", type=int, default=0, help="the mis2_lanes_per_vertex knob (0 = the library's choice)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mis2", "bench_mis2.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mis2 needs the GPU"
    src = os.path.join(ROOT, "kokkos-kernels_amd", "csrc", "kk_mis2.hip")
    stamp = hashlib.sha256(open(src, "rb").read()).hexdigest()[:12]
    try:
        for name in a.cases.split(","):
            line = run(name, a.lanes)
            line["kk_mis2_hip"] = stamp
            text = json.dumps(line)
            print(text, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(text + "\n")
    finally:
        kk.torch_backend().lib.kkamd_set_default(b"mis2_lanes_per_vertex", 0)


if __name__ == "__main__":
    main()
