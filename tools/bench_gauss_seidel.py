"""Multicolor Gauss-Seidel: symbolic, numeric and apply times of kk_gauss_seidel.hip against this library's own handle-less SpMV on the
same matrix in the same process.  One JSON line per run on stdout, appended to --out, stamped with the hash of kk_gauss_seidel.hip.

  python tools/bench_gauss_seidel.py [--stencil 27pt|7pt] [--n 100] [--dtype float64|float32] [--colors computed|parity] [--lanes 0]
                                     [--out profiles/gauss_seidel/bench_gauss_seidel.jsonl]

Matrix: the 27-point (or 7-point) stencil on n^3 points, x fastest, diagonal 26 (6), off-diagonals -1, columns ascending, int32 offsets.
--colors parity supplies the 8 (2) parity colours of the lattice instead of letting the library colour.
Times: the median of 20 after 3 warm-up calls, taken twice: host clock around one call that ends in a device synchronise (wall_ms) and
a pair of events on the stream around the same call (event_ms).  symbolic and numeric are single calls on the host clock.
Byte model of one apply with s sweeps (forward: s = 1, symmetric: s = 2 per iteration):
  s * (nnz (value + 4) + rows (8 + value) + rows 3 value)     the permuted matrix once per sweep: values, columns, row offsets, inverse
                                                              diagonal; Y read and X read and written once (the gathers of X are not
                                                              counted: they hit lines another row wrote)
  + rows 2 value + cols 4 value + (rows + 2 cols) 4           the permute passes: Y in, X in, X out, with their old_to_new reads"""
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


def medians_ms(fn, reps=20, warm=3):
    """(wall, event) medians of fn in ms"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    wall, event = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        event.append(e0.elapsed_time(e1))
    return statistics.median(wall), statistics.median(event)


def lattice(n, stencil, dtype):
    """the stencil's matrix on n^3 points and the lattice's parity colours (1-based)"""
    N = n * n * n
    i = torch.arange(N, dtype=torch.int32, device="cuda")
    x, y, z = i % n, (i // n) % n, i // (n * n)
    offs = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if stencil == "27pt" or abs(dx) + abs(dy) + abs(dz) <= 1]
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
        val[p] = float(len(offs) - 1) if d == 0 else -1.0
        pos += ok
    parity = (1 + x % 2 + 2 * (y % 2) + 4 * (z % 2)) if stencil == "27pt" else (1 + (x + y + z) % 2)
    return kk.CrsMatrix(N, N, rm, ent, val), parity.int().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stencil", default="27pt", choices=["27pt", "7pt"])
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--dtype", default="float64", choices=["float64", "float32"])
    ap.add_argument("--colors", default="computed", choices=["computed", "parity"])
    ap.add_argument("--lanes", type=int, default=0, help="the lanes_per_row knob (0 = the library's choice)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauss_seidel", "bench_gauss_seidel.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gauss_seidel needs the GPU"
    src = os.path.join(ROOT, "kokkos-kernels_amd", "csrc", "kk_gauss_seidel.hip")
    stamp = hashlib.sha256(open(src, "rb").read()).hexdigest()[:12]
    dtype = {"float64": torch.float64, "float32": torch.float32}[a.dtype]
    vsz = 8 if a.dtype == "float64" else 4
    A, parity = lattice(a.n, a.stencil, dtype)
    n, nnz = A.numRows(), A.nnz()
    rm, ent, val = A.graph.row_map, A.graph.entries, A.values
    y = torch.rand(n, dtype=dtype, device="cuda") * 2 - 1
    x = torch.zeros(n, dtype=dtype, device="cuda")
    out = torch.zeros(n, dtype=dtype, device="cuda")
    spmv_wall, spmv_event = medians_ms(lambda: kk.spmv("N", 1.0, A, y, 0.0, out))

    kh = kk.KokkosKernelsHandle(A.backend)
    kh.create_gs_handle("GS_DEFAULT")
    gh = kh.get_gs_handle()
    gh.set("lanes_per_row", a.lanes)
    kk.gauss_seidel_symbolic(kh, n, n, rm, ent, True, parity if a.colors == "parity" else None)     # warm-up: first-use costs of the kernels
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kk.gauss_seidel_symbolic(kh, n, n, rm, ent, True, parity if a.colors == "parity" else None)
    torch.cuda.synchronize()
    symbolic_ms = (time.perf_counter() - t0) * 1e3
    kk.gauss_seidel_numeric(kh, n, n, rm, ent, val)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kk.gauss_seidel_numeric(kh, n, n, rm, ent, val)
    torch.cuda.synchronize()
    numeric_ms = (time.perf_counter() - t0) * 1e3

    fwd_wall, fwd_event = medians_ms(lambda: kk.forward_sweep_gauss_seidel_apply(kh, n, n, rm, ent, val, x, y, True, True, 1.0, 1))
    sym_wall, sym_event = medians_ms(lambda: kk.symmetric_gauss_seidel_apply(kh, n, n, rm, ent, val, x, y, True, True, 1.0, 1))
    sym4_wall, sym4_event = medians_ms(lambda: kk.symmetric_gauss_seidel_apply(kh, n, n, rm, ent, val, x, y, True, True, 1.0, 4))
    # the residual of 4 symmetric iterations from x = 0, against the right-hand side's norm: the smoother smooths
    kk.spmv("N", 1.0, A, x, 0.0, out)
    rel_res = float(((out - y).norm() / y.norm()).item())

    sweep = nnz * (vsz + 4) + n * (8 + vsz) + n * 3 * vsz
    permute = n * 2 * vsz + n * 4 * vsz + 3 * n * 4
    per_sweep_event = (sym4_event - sym_event) / 6.0        # 4 iterations hold 6 sweeps more than 1, and the same permute passes
    line = {"matrix": "%s_%d^3" % (a.stencil, a.n), "rows": n, "nnz": nnz, "offset": "int32", "value": a.dtype, "colors": a.colors, "lanes_per_row": a.lanes,
            "symbolic_ms": round(symbolic_ms, 3), "numeric_ms": round(numeric_ms, 4),
            "forward_apply_wall_ms": round(fwd_wall, 4), "forward_apply_event_ms": round(fwd_event, 4),
            "symmetric_apply_wall_ms": round(sym_wall, 4), "symmetric_apply_event_ms": round(sym_event, 4),
            "symmetric_per_iteration_event_ms": round((sym4_event - sym_event) / 3.0, 4), "sweep_alone_event_ms": round(per_sweep_event, 4),
            "spmv_wall_ms": round(spmv_wall, 4), "spmv_event_ms": round(spmv_event, 4),
            "forward_apply_over_spmv": round(fwd_event / spmv_event, 3), "sweep_alone_over_spmv": round(per_sweep_event / spmv_event, 3),
            "num_colors": gh.get_num_colors(), "coloring_rounds": gh.get("coloring_rounds"), "launches": gh.get("launches"),
            "chain_launches": gh.get("chain_launches"), "max_level_rows": gh.get("max_level_rows"), "plan_bytes": gh.get("plan_bytes"),
            "model_bytes_forward_apply": sweep + permute, "frac_of_8TBs_forward_apply": round((sweep + permute) / (fwd_event * 1e-3) / HBM_PEAK, 5),
            "model_bytes_sweep": sweep, "frac_of_8TBs_sweep_alone": round(sweep / (per_sweep_event * 1e-3) / HBM_PEAK, 5),
            "relative_residual_after_4_symmetric": rel_res, "kk_gauss_seidel_hip": stamp}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")
    kh.destroy_gs_handle()


if __name__ == "__main__":
    main()
