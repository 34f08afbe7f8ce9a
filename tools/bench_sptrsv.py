"""Sparse triangular solve: symbolic and solve times of the level-scheduled kernels (kk_sptrsv.hip) against this library's own
handle-less SpMV on the same triangle, with the knob sweeps of DESIGN.md 4.5.  One JSON line per run on stdout (and appended to
the file given with --out), each stamped with the hash of kk_sptrsv.hip.

  python tools/bench_sptrsv.py [--sizes 100,200,300] [--random-rows 5000000] [--out profiles/sptrsv/bench_sptrsv.jsonl]

Matrices: the lower triangle (diagonal included) of the 27-point FE Laplacian on n^3 points -- n + 6 (n - 1) levels -- and a random
lower triangle with 0-3 off-diagonal entries per row drawn from all earlier rows (few, wide levels and a narrow tail).
Times: host clock around one call that ends in a device synchronise; the median of 20 after 3 warm-up calls.
Byte model of one solve: nnz (value + 4) + rows (offset + 4 + 4 + 2 value): values and entries once, row_map, the grouped row list,
the diagonal position, b read and x written once; the gathers of x are not counted (they hit lines another row wrote)."""
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
HBM_PEAK = 8.0e12


def median_ms(fn, reps=20, warm=3):
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


def lattice_lower(n):
    """lower triangle, diagonal included, of the 27-point stencil on n^3 points (x fastest): diagonal 26, off-diagonals -1, columns
    ascending.  Built here and not cut out of kkamd_gen_laplace's matrix: that one carries the reference generator's boundary rows
    (zero and unit diagonals), which a triangular solve cannot use."""
    N = n * n * n
    i = torch.arange(N, dtype=torch.int32, device="cuda")
    x, y, z = i % n, (i // n) % n, i // (n * n)
    offs = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx + n * (dy + n * dz) <= 0]
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
        val[p] = 26.0 if d == 0 else -1.0
        pos += ok
    return kk.CrsMatrix(N, N, rm, ent, val)


def random_lower(n, seed=200):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    idx = torch.arange(n, device="cuda")
    cnt = torch.minimum(torch.randint(0, 4, (n,), device="cuda", generator=g), idx)
    rows = torch.repeat_interleave(idx, cnt)
    cols = (torch.rand(rows.shape[0], device="cuda", dtype=torch.float64, generator=g) * rows).long()
    off = torch.rand(rows.shape[0], device="cuda", dtype=torch.float64, generator=g) * 2 - 1
    s = torch.zeros(n, dtype=torch.float64, device="cuda").index_add_(0, rows, off.abs())
    r = torch.cat([rows, idx]); c = torch.cat([cols, idx]); v = torch.cat([off, 2.0 * (1.0 + s)])
    order = torch.sort(r, stable=True).indices
    rm = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    rm[1:] = torch.cumsum(cnt + 1, 0)
    return kk.CrsMatrix(n, n, rm, c[order].int().contiguous(), v[order].contiguous())


def run(name, L, stamp, out, sweeps):
    n, nnz = L.numRows(), L.nnz()
    rm, ent, val = L.graph.row_map, L.graph.entries, L.values
    b = torch.rand(n, dtype=torch.float64, device="cuda") * 2 - 1
    x = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    spmv_ms = median_ms(lambda: kk.spmv("N", 1.0, L, b, 0.0, y))
    kh = kk.KokkosKernelsHandle(L.backend)
    kh.create_sptrsv_handle("SEQLVLSCHD_TP1CHAIN", n, True)
    th = kh.get_sptrsv_handle()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kk.sptrsv_symbolic(kh, rm, ent)
    torch.cuda.synchronize()
    symbolic_ms = (time.perf_counter() - t0) * 1e3
    model = nnz * (8 + 4) + n * (4 + 4 + 4 + 2 * 8)
    for knobs in [{}] + sweeps:
        for key in ("lanes_per_row", "chain_rows", "chain_levels"):
            th.set(key, knobs.get(key, {"lanes_per_row": 0, "chain_rows": 64, "chain_levels": 1024}[key]))
        solve_ms = median_ms(lambda: kk.sptrsv_solve(kh, rm, ent, val, b, x))
        kk.spmv("N", 1.0, L, x, 0.0, y)
        line = {"matrix": name, "rows": n, "nnz": nnz, "offset": "int32", "value": "float64", "algorithm": "SEQLVLSCHD_TP1CHAIN",
                "knobs": knobs, "symbolic_ms": round(symbolic_ms, 3), "solve_ms": round(solve_ms, 4), "spmv_ms": round(spmv_ms, 4),
                "levels": th.get_num_levels(), "max_level_rows": th.get("max_level_rows"), "launches": th.get("launches"),
                "chain_launches": th.get("chain_launches"), "chained_levels": th.get("chained_levels"), "plan_bytes": th.get("plan_bytes"),
                "model_bytes": model, "frac_of_8TBs": round(model / (solve_ms * 1e-3) / HBM_PEAK, 5),
                "residual_max": float((y - b).abs().max().item()), "kk_sptrsv_hip": stamp}
        text = json.dumps(line)
        print(text, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(text + "\n")
    kh.destroy_sptrsv_handle()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,200,300")
    ap.add_argument("--random-rows", type=int, default=5000000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sptrsv needs the GPU"
    src = os.path.join(ROOT, "kokkos-kernels_amd", "csrc", "kk_sptrsv.hip")
    stamp = hashlib.sha256(open(src, "rb").read()).hexdigest()[:12]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    sizes = [int(s) for s in a.sizes.split(",") if s]
    for n in sizes:
        sweeps = []
        if n == max(sizes):
            sweeps = [{"chain_rows": c} for c in (0, 64, 256, 1024)] + [{"lanes_per_row": l} for l in (4, 8, 16)]
        run("27pt_lower_%d^3" % n, lattice_lower(n), stamp, a.out, sweeps)
    if a.random_rows:
        run("random_lower_%d" % a.random_rows, random_lower(a.random_rows), stamp, a.out, [])


if __name__ == "__main__":
    main()
