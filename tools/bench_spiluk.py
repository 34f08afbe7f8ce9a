"""ILU(k): symbolic and numeric times of the level-scheduled factorisation (kk_spiluk.hip), with -- measured in the same run -- this
library's sptrsv_solve on the resulting L and one handle-less SpMV of A, and the knob sweeps of DESIGN.md 4.6.  One JSON line per run
on stdout (and appended to the file given with --out), each stamped with the hash of kk_spiluk.hip.

  python tools/bench_spiluk.py [--cases 27:300:0,27:300:1,7:300:0] [--sweep] [--out profiles/spiluk/bench_spiluk.jsonl]

A case is points:n:fill_lev: the 27-point (diagonal 26, off-diagonals -1) or 7-point (diagonal 6) stencil on n^3 points, fp64, int32
offsets.  --sweep adds lanes_per_row and chain_rows sweeps on the first case.
Times: host clock around one call that ends in a device synchronise; numeric, solve and SpMV are the median of 10 after 2 warm-up
calls; the symbolic phase runs once, its host fill loop and the rest (copies, level sets on the device) reported separately as the
library's handle records them."""
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


def median_ms(fn, reps=10, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def lattice(n, points):
    """the 27-point or 7-point stencil on n^3 points (x fastest), columns ascending: diagonal points - 1, off-diagonals -1"""
    N = n * n * n
    i = torch.arange(N, dtype=torch.int32, device="cuda")
    x, y, z = i % n, (i // n) % n, i // (n * n)
    offs = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if points == 27 or abs(dx) + abs(dy) + abs(dz) <= 1]
    offs.sort(key=lambda o: o[0] + n * (o[1] + n * o[2]))
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
    val = torch.empty(nnz, dtype=torch.float64, device="cuda")
    pos = rm[:-1].clone().long()
    for (dx, dy, dz), ok in zip(offs, masks):
        d = dx + n * (dy + n * dz)
        p = pos[ok]
        ent[p] = (i[ok] + d)
        val[p] = float(points - 1) if d == 0 else -1.0
        pos += ok
    return kk.CrsMatrix(N, N, rm, ent, val)


def run(name, A, fill_lev, stamp, out, sweeps):
    n, nnz = A.numRows(), A.nnz()
    rm, ent, val = A.graph.row_map, A.graph.entries, A.values
    x = torch.rand(n, dtype=torch.float64, device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    spmv_ms = median_ms(lambda: kk.spmv("N", 1.0, A, x, 0.0, y))
    cap = nnz * (1 + 2 * fill_lev) + n                       # generous: the symbolic phase names the true count when it is not
    kh = kk.KokkosKernelsHandle(A.backend)
    kh.create_spiluk_handle("SEQLVLSCHD_TP1", n, cap, cap)
    ih = kh.get_spiluk_handle()
    L_rm, U_rm = torch.empty_like(rm), torch.empty_like(rm)
    L_ent = torch.empty(cap, dtype=torch.int32, device="cuda"); U_ent = torch.empty(cap, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kk.spiluk_symbolic(kh, fill_lev, rm, ent, L_rm, L_ent, U_rm, U_ent)
    torch.cuda.synchronize()
    symbolic_ms = (time.perf_counter() - t0) * 1e3
    nnzL, nnzU = ih.get_nnzL(), ih.get_nnzU()
    L_ent, U_ent = L_ent[:nnzL].clone(), U_ent[:nnzU].clone()
    L_val = torch.full((nnzL,), float("nan"), dtype=torch.float64, device="cuda")
    U_val = torch.full((nnzU,), float("nan"), dtype=torch.float64, device="cuda")
    numeric = lambda: kk.spiluk_numeric(kh, fill_lev, rm, ent, val, L_rm, L_ent, L_val, U_rm, U_ent, U_val)
    base = None
    for knobs in [{}] + sweeps:
        for key in ("lanes_per_row", "chain_rows", "chain_levels"):
            ih.set(key, knobs.get(key, {"lanes_per_row": 0, "chain_rows": 64, "chain_levels": 1024}[key]))
        numeric_ms = median_ms(numeric)
        line = {"matrix": name, "fill_lev": fill_lev, "rows": n, "nnz": nnz, "nnzL": nnzL, "nnzU": nnzU, "offset": "int32", "value": "float64",
                "knobs": knobs, "lanes_in_use": ih.get("lanes_in_use"), "numeric_ms": round(numeric_ms, 4), "levels": ih.get_num_levels(),
                "max_level_rows": ih.get("max_level_rows"), "launches": ih.get("launches"), "chain_launches": ih.get("chain_launches"),
                "chained_levels": ih.get("chained_levels"), "numeric_us_per_level": round(numeric_ms * 1e3 / max(ih.get_num_levels(), 1), 3),
                "plan_bytes": ih.get("plan_bytes"), "kk_spiluk_hip": stamp}
        if base is None:
            # the factors as the triangular solve's input, and that L U reproduces A's diagonal-block action closely enough to be a preconditioner
            assert bool(torch.isfinite(L_val).all()) and bool(torch.isfinite(U_val).all())
            th = kk.KokkosKernelsHandle(A.backend)
            th.create_sptrsv_handle("SEQLVLSCHD_TP1CHAIN", n, True)
            kk.sptrsv_symbolic(th, L_rm, L_ent)
            b = torch.rand(n, dtype=torch.float64, device="cuda")
            z = torch.empty_like(b)
            solve_ms = median_ms(lambda: kk.sptrsv_solve(th, L_rm, L_ent, L_val, b, z))
            th.destroy_sptrsv_handle()
            base = {"symbolic_ms": round(symbolic_ms, 1), "symbolic_host_fill_ms": round(ih.get("symbolic_fill_us") / 1e3, 1),
                    "symbolic_copies_and_device_levels_ms": round(ih.get("symbolic_other_us") / 1e3, 1),
                    "sptrsv_solve_L_ms": round(solve_ms, 4), "spmv_A_ms": round(spmv_ms, 4)}
        line.update(base)
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
    kh.destroy_spiluk_handle()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="27:300:0,27:300:1,7:300:0")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spiluk needs the GPU"
    src = os.path.join(ROOT, "kokkos-kernels_amd", "csrc", "kk_spiluk.hip")
    stamp = hashlib.sha256(open(src, "rb").read()).hexdigest()[:12]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for k, case in enumerate(c for c in a.cases.split(",") if c):
        points, n, fill_lev = (int(v) for v in case.split(":"))
        sweeps = []
        if a.sweep and k == 0:
            sweeps = [{"lanes_per_row": l} for l in (4, 8, 16, 32)] + [{"chain_rows": c} for c in (0, 256, 1024)]
        run("%dpt_%d^3" % (points, n), lattice(n, points), fill_lev, stamp, a.out, sweeps)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
