"""ParILUT: per-step times of one numeric call (kk_par_ilut.hip) on the 7-point and 27-point lattices, with -- measured in the same process,
for scale -- this library's spiluk_numeric (k = 0) on the same matrix.  One JSON line per case on stdout (and appended to the file given
with --out), each stamped with the hash of kk_par_ilut.hip.

  python tools/bench_par_ilut.py [--cases 7:100,27:100] [--max-iter 5] [--out profiles/par_ilut/bench_par_ilut.jsonl]

A case is points:n: the 27-point (diagonal 26, off-diagonals -1) or 7-point (diagonal 6) stencil on n^3 points, fp64, int32 offsets.
Times: numeric_ms is the host clock around one call (it synchronises), the median of 3 after 1 warm-up call; the step times come from a
further call under the knob "profile" (a stream synchronisation and a host clock reading after every step, summed over the iterations), so
their sum exceeds numeric_ms by the synchronisations.  max_iter is capped (default 5) so that the counts are comparable between cases."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import kk_loader  # noqa: E402
from bench_spiluk import lattice, median_ms  # noqa: E402

kk = kk_loader.load()
STEPS = ("product", "candidates", "transpose", "sweep", "select", "filter", "residual")


def run(name, A, max_iter, stamp, out):
    n, nnz = A.numRows(), A.nnz()
    rm, ent, val = A.graph.row_map, A.graph.entries, A.values
    # ILU(0) by the level-scheduled factorisation, for scale
    kh0 = kk.KokkosKernelsHandle(A.backend)
    kh0.create_spiluk_handle("SEQLVLSCHD_TP1", n, nnz + n, nnz + n)
    L_rm, U_rm = torch.empty_like(rm), torch.empty_like(rm)
    L_ent = torch.empty(nnz + n, dtype=torch.int32, device="cuda"); U_ent = torch.empty(nnz + n, dtype=torch.int32, device="cuda")
    kk.spiluk_symbolic(kh0, 0, rm, ent, L_rm, L_ent, U_rm, U_ent)
    L_val = torch.empty(nnz + n, dtype=torch.float64, device="cuda"); U_val = torch.empty(nnz + n, dtype=torch.float64, device="cuda")
    spiluk_ms = median_ms(lambda: kk.spiluk_numeric(kh0, 0, rm, ent, val, L_rm, L_ent, L_val, U_rm, U_ent, U_val), reps=5, warm=1)
    spiluk_levels = kh0.get_spiluk_handle().get_num_levels()
    kh0.destroy_spiluk_handle()
    del L_ent, U_ent, L_val, U_val
    # ParILUT
    kh = kk.KokkosKernelsHandle(A.backend)
    kh.create_par_ilut_handle(max_iter=max_iter)
    ih = kh.get_par_ilut_handle()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kk.par_ilut_symbolic(kh, rm, ent, L_rm, U_rm)
    torch.cuda.synchronize()
    symbolic_ms = (time.perf_counter() - t0) * 1e3
    numeric_ms = median_ms(lambda: kk.par_ilut_numeric(kh, rm, ent, val, L_rm, U_rm), reps=3, warm=1)
    line = {"matrix": name, "rows": n, "nnz": nnz, "offset": "int32", "value": "float64", "max_iter": max_iter, "nnzL": ih.get_nnzL(), "nnzU": ih.get_nnzU(),
            "nnzL_out": ih.get("nnzL_out"), "nnzU_out": ih.get("nnzU_out"), "num_iters": ih.get_num_iters(), "end_rel_res": ih.get_end_rel_res(),
            "lanes_in_use": ih.get("lanes_in_use"), "symbolic_ms": round(symbolic_ms, 2), "numeric_ms": round(numeric_ms, 3),
            "host_syncs": ih.get("host_syncs"), "launches": ih.get("launches"), "plan_bytes": ih.get("plan_bytes"),
            "spiluk0_numeric_ms": round(spiluk_ms, 3), "spiluk0_levels": spiluk_levels, "kk_par_ilut_hip": stamp}
    ih.set("profile", 1)
    kk.par_ilut_numeric(kh, rm, ent, val, L_rm, U_rm)
    for s in STEPS:
        line[s + "_ms"] = round(ih.get_real(s + "_ms"), 3)
    kh.destroy_par_ilut_handle()
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="7:100,27:100")
    ap.add_argument("--max-iter", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_par_ilut needs the GPU"
    src = os.path.join(ROOT, "kokkos-kernels_amd", "csrc", "kk_par_ilut.hip")
    stamp = hashlib.sha256(open(src, "rb").read()).hexdigest()[:12]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for case in (c for c in a.cases.split(",") if c):
        points, n = (int(v) for v in case.split(":"))
        run("%dpt_%d^3" % (points, n), lattice(n, points), a.max_iter, stamp, a.out)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
