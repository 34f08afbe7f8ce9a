"""Restarted GMRES: per-iteration times of the SpMV, the orthogonalisation and the preconditioner inside kkamd_gmres_solve, for the
variants of kk_gmres.hip in one process.  One JSON line per variant on stdout, appended to --out, stamped with the hash of kk_gmres.hip.

  python tools/bench_gmres.py [--n 100] [--dtype float64|float32] [--m 50] [--reps 5] [--fuse-max-k 0] [--out profiles/gmres/bench_gmres.jsonl]

Matrix: the 27-point stencil on n^3 points (diagonal 26, off-diagonals -1), int32 offsets; b uniform in (-1, 1), x0 = 0.  tol = 1e-30 and
max_restart = 0, so that every solve runs exactly one cycle of m iterations.  Variants: CGS2 with "fuse" 1 and 0, alternating, and MGS,
each without a preconditioner and with ILU(0) (the library's spiluk) as LUPrec.
Times: the knob "profile" puts four events per iteration on the stream (before the preconditioner, before the SpMV, after it, after the
normalise kernel); reported per iteration j is the median over --reps solves after one warm-up solve.  solve_wall_ms is the host clock
around the whole solve, which synchronises.
Byte model of the orthogonalisation of iteration j, k = j + 1 columns: (3 or 4) k n value + 6 n value -- V read three ("fuse" 1, k <= 64)
or four times, w read and written by the two updates, read by the first dot (the second reads it too when not fused) and by the normalise
kernel, which writes the new column."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import kk_loader  # noqa: E402

kk = kk_loader.load()
HBM_PEAK = 8.0e12
SHOW = (0, 4, 8, 16, 24, 32, 40, 49)


def lattice(n, dtype):
    """the 27-point stencil on n^3 points, x fastest: diagonal 26, off-diagonals -1, columns ascending (as tools/bench_gauss_seidel.py)"""
    N = n * n * n
    i = torch.arange(N, dtype=torch.int32, device="cuda")
    x, y, z = i % n, (i // n) % n, i // (n * n)
    offs = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    masks = []
    cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
    for dx, dy, dz in offs:
        ok = (x + dx >= 0) & (x + dx < n) & (y + dy >= 0) & (y + dy < n) & (z + dz >= 0) & (z + dz < n)
        masks.append(ok)
        cnt += ok
    rm = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
    rm[1:] = torch.cumsum(cnt, 0)
    nnz = int(rm[-1].item())
    ent = torch.empty(nnz, dtype=torch.int32, device="cuda")
    val = torch.empty(nnz, dtype=dtype, device="cuda")
    pos = rm[:-1].clone().long()
    for (dx, dy, dz), ok in zip(offs, masks):
        d = dx + n * (dy + n * dz)
        p = pos[ok]
        ent[p] = (i[ok] + d)
        val[p] = 26.0 if d == 0 else -1.0
        pos += ok
    return kk.CrsMatrix(N, N, rm, ent, val)


def ilu0_precond(A, be, dtype):
    n, nnz = A.numRows(), A.nnz()
    kh = kk.KokkosKernelsHandle(be)
    kh.create_spiluk_handle("SEQLVLSCHD_TP1", n, nnz, nnz)
    Lrm, Urm = be.empty(n + 1, np.int32), be.empty(n + 1, np.int32)
    Le, Ue = be.empty(nnz + n, np.int32), be.empty(nnz + n, np.int32)
    kk.spiluk_symbolic(kh, 0, A.graph.row_map, A.graph.entries, Lrm, Le, Urm, Ue)
    sh = kh.get_spiluk_handle()
    nl, nu = sh.get_nnzL(), sh.get_nnzU()
    Lv, Uv = be.empty(nnz + n, dtype), be.empty(nnz + n, dtype)
    kk.spiluk_numeric(kh, 0, A.graph.row_map, A.graph.entries, A.values, Lrm, Le, Lv, Urm, Ue, Uv)
    torch.cuda.synchronize()
    kh.destroy_spiluk_handle()
    return kk.LUPrec(kk.CrsMatrix(n, n, Lrm, Le[:nl], Lv[:nl], backend=be), kk.CrsMatrix(n, n, Urm, Ue[:nu], Uv[:nu], backend=be))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--m", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fuse-max-k", type=int, default=0, help="the fuse_max_k knob (0 = the library's default)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmres", "bench_gmres.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gmres needs the GPU"
    src = os.path.join(ROOT, "kokkos-kernels_amd", "csrc", "kk_gmres.hip")
    stamp = hashlib.sha256(open(src, "rb").read()).hexdigest()[:12]
    dtype = np.float64 if a.dtype == "float64" else np.float32
    vsz = np.dtype(dtype).itemsize
    be = kk.torch_backend()
    A = lattice(a.n, torch.float64 if dtype is np.float64 else torch.float32)
    n, nnz = A.numRows(), A.nnz()
    torch.manual_seed(0)
    B = (torch.rand(n, dtype=torch.float64, device="cuda") * 2 - 1).to(torch.float64 if dtype is np.float64 else torch.float32)
    lu = ilu0_precond(A, be, dtype)
    spmv_bytes = nnz * (vsz + 4) + n * (4 + 2 * vsz)
    shown = [j for j in SHOW if j < a.m]

    variants = [("CGS2", 1), ("CGS2", 0), ("MGS", 1)]
    samples = {}
    kh = kk.KokkosKernelsHandle(be)
    kh.create_gmres_handle(a.m, 1e-30, 0)
    gh = kh.get_gmres_handle()
    gh.set("profile", 1)
    if a.fuse_max_k:
        gh.set("fuse_max_k", a.fuse_max_k)
    for prec_name, prec in (("none", None), ("ilu0", lu)):
        for rep in range(a.reps + 1):                                   # rep 0 warms every variant up; the variants alternate inside a rep
            for ortho, fuse in variants:
                gh.set_ortho(ortho); gh.set("fuse", fuse)
                X = torch.zeros_like(B)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                kk.gmres(kh, A, B, X, prec)                      # a breakdown or NaN raises: a bench of a solve that failed reports nothing
                wall = (time.perf_counter() - t0) * 1e3
                if rep == 0:
                    continue
                s = samples.setdefault((prec_name, ortho, fuse), {"wall": [], "spmv": [], "ortho": [], "precond": []})
                s["wall"].append(wall)
                for key in ("spmv", "ortho", "precond"):
                    s[key].append(gh.export(key + "_ms"))
                s["iters"], s["syncs"], s["launches"], s["res"] = gh.get_num_iters(), gh.get("host_syncs"), gh.get("launches"), gh.get_end_rel_res()
                s["fused"] = gh.get("last_fused")
    for (prec_name, ortho, fuse), s in samples.items():
        med = {key: np.median(np.array(s[key]), axis=0) for key in ("spmv", "ortho", "precond")}
        fmk = gh.get("fuse_max_k")
        passes = [3 if (ortho == "CGS2" and fuse and j + 1 <= fmk) else (4 if ortho == "CGS2" else 2) for j in range(a.m)]
        model = [(passes[j] * (j + 1) * n * vsz + (6 if ortho == "CGS2" else 3 * (j + 1) + 3) * n * vsz) for j in range(a.m)]
        line = {"matrix": "27pt_%d^3" % a.n, "rows": n, "nnz": nnz, "value": a.dtype, "m": a.m, "precond": prec_name, "ortho": ortho, "fuse": fuse, "fuse_max_k": fmk,
                "last_fused": s["fused"], "iterations": s["iters"], "host_syncs": s["syncs"], "launches": s["launches"], "reps": a.reps,
                "solve_wall_ms": round(statistics.median(s["wall"]), 3), "solve_wall_ms_min_max": [round(min(s["wall"]), 3), round(max(s["wall"]), 3)],
                "sum_spmv_ms": round(float(med["spmv"].sum()), 3), "sum_ortho_ms": round(float(med["ortho"].sum()), 3),
                "sum_precond_ms": round(float(med["precond"].sum()), 3), "j": shown,
                "spmv_ms": [round(float(med["spmv"][j]), 4) for j in shown], "ortho_ms": [round(float(med["ortho"][j]), 4) for j in shown],
                "precond_ms": [round(float(med["precond"][j]), 4) for j in shown],
                "ortho_model_bytes": [model[j] for j in shown],
                "ortho_frac_of_8TBs": [round(model[j] / (float(med["ortho"][j]) * 1e-3) / HBM_PEAK, 4) for j in shown],
                "spmv_frac_of_8TBs": [round(spmv_bytes / (float(med["spmv"][j]) * 1e-3) / HBM_PEAK, 4) for j in shown],
                "end_rel_res": s["res"], "kk_gmres_hip": stamp}
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(text + "\n")
    kh.destroy_gmres_handle()


if __name__ == "__main__":
    main()
