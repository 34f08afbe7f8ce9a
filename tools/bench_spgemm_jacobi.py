"""spgemm_jacobi against spgemm_numeric on the same operands: what the prologue (a' = a * mult) and the epilogue (C += rows of B) add to the
numeric phase.  One JSON line per case on stdout, appended to --out, stamped with the hash of kk_spgemm.hip.

  python tools/bench_spgemm_jacobi.py [--cases 27pt_100,7pt_100] [--timeout 600] [--out profiles/spgemm_jacobi/bench_spgemm_jacobi.jsonl]

The GPU step is one child process (this file with --worker) under its own time limit; the parent never opens the GPU.

Cases, per lattice (27-point and 7-point on n^3 points, diagonal stored, columns strictly ascending, int32 offsets, fp64 values, diagonal 26 / 6
and -1 elsewhere): A * P with P the tentative prolongator of graph_mis2_aggregate's labels (one unit entry per row), and A * A.  omega = 2/3,
dinv = 1 / diagonal.  Each product has two handles with a symbolic phase and a C of their own, one for spgemm_numeric and one for spgemm_jacobi.
Times: a pair of events on the stream around each call (every call ends in a host synchronisation of its own); the first call is reported
apart (it writes entries(C) and allocates), then the median of 10 calls.
Byte model of the two added passes (the bisection probes of the epilogue are not counted):
  prologue  nnz(A) * 2 * value + rows * (2 * offset + value)
  epilogue  nnz(B rows) * (4 + 3 * value) + rows * 4 * offset
model_ratio = 1 + model bytes / 8 TB/s / numeric time: what the ratio would be if the added passes ran at the roofline the project quotes."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def model_bytes(nnz_a, nnz_b_rows, rows, value=8, offset=4):
    return nnz_a * 2 * value + rows * (2 * offset + value), nnz_b_rows * (4 + 3 * value) + rows * 4 * offset


def worker(cases, out):
    import torch
    import kk_loader
    from bench_mis2 import lattice

    kk = kk_loader.load()
    assert torch.cuda.is_available(), "bench_spgemm_jacobi needs the GPU"
    be = kk.torch_backend()
    src = os.path.join(ROOT, "kokkos-kernels_amd", "csrc", "kk_spgemm.hip")
    stamp = hashlib.sha256(open(src, "rb").read()).hexdigest()[:12]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def first_and_median(fn, reps=10):
        first = timed(fn)
        return first, statistics.median(timed(fn) for _ in range(reps))

    for name in cases:
        kind, size = name.split("_")
        n, rm, ent = lattice(int(size), kind)
        nnz = int(ent.shape[0])
        rows = torch.repeat_interleave(torch.arange(n, device="cuda"), (rm[1:] - rm[:-1]).long())
        diag = 26.0 if kind == "27pt" else 6.0
        val = torch.where(ent.long() == rows, torch.tensor(diag, dtype=torch.float64, device="cuda"), torch.tensor(-1.0, dtype=torch.float64, device="cuda"))
        A = kk.CrsMatrix(n, n, rm, ent, val.contiguous())
        labels, nagg = kk.graph_mis2_aggregate(rm, ent)
        P = kk.CrsMatrix(n, nagg, torch.arange(n + 1, dtype=torch.int32, device="cuda"), labels.contiguous(), torch.ones(n, dtype=torch.float64, device="cuda"))
        dinv = torch.full((n,), 1.0 / diag, dtype=torch.float64, device="cuda")
        for product, B in (("A*P", P), ("A*A", A)):
            line = {"lattice": name, "product": product, "rows": n, "nnz_A": nnz, "nnz_B": B.nnz(), "cols_B": B.numCols(), "offset": "int32", "value": "fp64",
                    "omega": 2.0 / 3.0}
            khn, khj = kk.KokkosKernelsHandle(be), kk.KokkosKernelsHandle(be)
            khn.create_spgemm_handle(); khj.create_spgemm_handle()
            Cn = kk.spgemm_symbolic(khn, A, False, B, False)
            Cj = kk.spgemm_symbolic(khj, A, False, B, False)
            line["nnz_C"] = Cn.nnz()
            line["numeric_first_ms"], line["numeric_ms"] = [round(v, 4) for v in first_and_median(lambda: kk.spgemm_numeric(khn, A, False, B, False, Cn))]
            line["jacobi_first_ms"], line["jacobi_ms"] = [round(v, 4) for v in first_and_median(lambda: kk.spgemm_jacobi(khj, A, False, B, False, Cj, 2.0 / 3.0, dinv))]
            # alternate the two once more: the spread of the same command on the same code
            line["numeric_ms_again"] = round(statistics.median(timed(lambda: kk.spgemm_numeric(khn, A, False, B, False, Cn)) for _ in range(10)), 4)
            line["jacobi_ms_again"] = round(statistics.median(timed(lambda: kk.spgemm_jacobi(khj, A, False, B, False, Cj, 2.0 / 3.0, dinv)) for _ in range(10)), 4)
            line["ratio"] = round(line["jacobi_ms"] / line["numeric_ms"], 3)
            line["ratio_again"] = round(line["jacobi_ms_again"] / line["numeric_ms_again"], 3)
            sh = khj.get_spgemm_handle()
            line["epilogue_lanes"], line["epilogue_fast"] = sh.get(24), sh.get(25)
            pro, epi = model_bytes(nnz, B.nnz(), n)
            line["model_prologue_bytes"], line["model_epilogue_bytes"] = pro, epi
            line["model_added_ms_at_8TBs"] = round((pro + epi) / 8e12 * 1e3, 4)
            line["model_ratio"] = round(1 + line["model_added_ms_at_8TBs"] / line["numeric_ms"], 3)
            line["added_ms"] = round(line["jacobi_ms"] - line["numeric_ms"], 4)
            line["kk_spgemm_hip"] = stamp
            text = json.dumps(line)
            print(text, flush=True)
            if out:
                os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
                with open(out, "a") as f:
                    f.write(text + "\n")
            khn.destroy_spgemm_handle(); khj.destroy_spgemm_handle()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="27pt_100,7pt_100")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spgemm_jacobi", "bench_spgemm_jacobi.jsonl"))
    ap.add_argument("--timeout", type=int, default=600, help="seconds the GPU step may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.cases.split(","), a.out)
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--cases", a.cases, "--out", a.out], timeout=a.timeout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
