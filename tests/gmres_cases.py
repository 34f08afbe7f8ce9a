"""Generated inputs, the restated reference loop and the shared checks of the GMRES tests (CPU only; used by test_emu_gmres.py and
test_gpu_gmres.py).

Cases (`small` cuts them to emulator size):
  diag5   diag of 1..5, each `rep` times (200; small 8), b = 1: exactly 5 iterations for m >= 5, restarts for m = 3
  tri     tridiagonal (4, -1), n = 513 (small 65); with its exact L, U as LUPrec one iteration (ILU(0) of a tridiagonal is exact)
  conv2d  non-symmetric 5-point stencil on 12 x 11 (small 6 x 5): 4 on the diagonal, -1.5 / -0.5 west / east, -1.25 / -0.75 south /
          north, b = 1; m in {50, 10, 4}; with the Jacobi MatrixPrec; with ILU(0) as LUPrec
  edge    b = 0 with x0 != 0; x0 already the solution; n = 1

restated_gmres is sparse/impl/KokkosSparse_gmres_impl.hpp:59-329 line by line in numpy, every scalar held in the value type; it records
every shortRelRes and relRes it compares with tol.  A case's margin is the smallest max(v / tol, tol / v) over those values.  tol is 1e-8
(fp64) / 1e-4 (fp32) when that leaves a margin of 1.5, else the geometric mean of the nearest two consecutive short residuals that are a
factor 2.3 apart (for conv2d with m = 10 in fp64 the nearest such gap is at 2.7e-6; every other tol is within a factor 10 of the target).

Kernel data: signed integers below 2^b times 2^-4.  V, h, w and d are such values; w_in = d - alpha V h, so that the updated vector is d
exactly.  Every partial sum is then a multiple of 2^-8 (dot V^T w, update V h, second product V^T d, sum d^2) with absolute value
below n 2^(2b - 8), k 2^(2b - 8) resp. (2k + 1) 2^(2b - 8) for w_in: b = min((p - 1 - ceil(log2 n)) / 2, (p - 3 - ceil(log2 k)) / 2)
rounded down (p = 53 / 24 significand bits) makes each of them representable, whatever the order of summation.
"""
import ctypes as C
import functools
import math
import types

import numpy as np
import pytest

DTYPES = (np.float64, np.float32)
UNIT = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
PBITS = {np.float64: 53, np.float32: 24}
TARGET_TOL = {np.float64: 1e-8, np.float32: 1e-4}
LD = np.longdouble


def gamma(k, dtype):
    u = UNIT[dtype]
    return k * u / (1 - k * u)


# ---------------------------------------------------------------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------------------------------------------------------------

def dense_to_crs(D):
    n = D.shape[0]
    rm, ent, val = [0], [], []
    for i in range(n):
        cols = np.nonzero(D[i])[0]
        ent.extend(cols.tolist()); val.extend(D[i, cols].tolist()); rm.append(len(ent))
    return np.array(rm, dtype=np.int64), np.array(ent, dtype=np.int32), np.array(val, dtype=np.float64)


def ilu0(D):
    """ILU(0) on the pattern of D (IKJ), as dense L (unit diagonal) and U"""
    n = D.shape[0]
    W = D.astype(np.float64).copy()
    pat = D != 0
    for i in range(1, n):
        for k in np.nonzero(pat[i, :i])[0]:
            W[i, k] = W[i, k] / W[k, k]
            for j in np.nonzero(pat[i, k + 1:])[0] + k + 1:
                if pat[k, j]:
                    W[i, j] -= W[i, k] * W[k, j]
    return np.tril(W, -1) + np.eye(n), np.triu(W)


class Case:
    """A (dense float64, values exact in fp32), b, x0, the restart length, the preconditioner kind (None, "jacobi", "lu")"""

    def __init__(self, name, D, b, x0, m, precond=None, max_restart=50):
        self.name, self.D, self.b, self.x0, self.m, self.precond, self.max_restart = name, D, b, x0, m, precond, max_restart
        self.n = D.shape[0]
        self.row_map, self.entries, self.values = dense_to_crs(D)
        self.row_len = np.diff(self.row_map)
        if precond == "jacobi":
            self.Minv = np.diag(1.0 / np.diag(D))
        elif precond == "lu":
            self.L, self.U = ilu0(D)

    def __repr__(self):
        return self.name

    def apply_M(self, dtype):
        """v -> M v in the value type, or None"""
        if self.precond == "jacobi":
            dinv = np.diag(self.Minv).astype(dtype)
            return lambda v: dinv * v
        if self.precond == "lu":
            L, U = self.L.astype(dtype), self.U.astype(dtype)

            def solve(v):
                n = len(v)
                y = np.zeros(n, dtype)
                for i in range(n):
                    y[i] = (v[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
                z = np.zeros(n, dtype)
                for i in range(n - 1, -1, -1):
                    z[i] = (y[i] - np.dot(U[i, i + 1:], z[i + 1:])) / U[i, i]
                return z
            return solve
        return None

    def M_dense(self):
        if self.precond == "jacobi":
            return self.Minv
        if self.precond == "lu":
            return np.linalg.inv(self.U) @ np.linalg.inv(self.L)
        return np.eye(self.n)


def _tri(n):
    return 4.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


def _conv2d(nx, ny):
    n = nx * ny
    D = np.zeros((n, n))
    for y in range(ny):
        for x in range(nx):
            i = y * nx + x
            D[i, i] = 4.0
            if x > 0: D[i, i - 1] = -1.5
            if x < nx - 1: D[i, i + 1] = -0.5
            if y > 0: D[i, i - nx] = -1.25
            if y < ny - 1: D[i, i + nx] = -0.75
    return D


@functools.lru_cache(maxsize=None)
def cases(small):
    rep = 8 if small else 200
    nt = 65 if small else 513
    nx, ny = (6, 5) if small else (12, 11)
    rng = np.random.default_rng(7)
    out = []
    Dd = np.diag(np.repeat(np.arange(1.0, 6.0), rep))
    for m in (50, 5, 3):
        out.append(Case("diag5-m%d" % m, Dd, np.ones(5 * rep), np.zeros(5 * rep), m))
    Dt = _tri(nt)
    bt = np.ones(nt)
    out.append(Case("tri", Dt, bt, np.zeros(nt), 50))
    out.append(Case("tri-lu", Dt, bt, np.zeros(nt), 50, "lu"))
    Dc = _conv2d(nx, ny)
    bc = np.ones(nx * ny)
    for m in (50, 10, 4):
        out.append(Case("conv2d-m%d" % m, Dc, bc, np.zeros(nx * ny), m))
    out.append(Case("conv2d-jacobi", Dc, bc, np.zeros(nx * ny), 50, "jacobi"))
    out.append(Case("conv2d-lu", Dc, bc, np.zeros(nx * ny), 50, "lu"))
    out.append(Case("edge-b0", Dt[:17, :17], np.zeros(17), np.arange(1.0, 18.0), 50))
    xs = np.round(rng.uniform(-4, 4, 5 * rep))
    out.append(Case("edge-x0-solution", Dd, Dd @ xs, xs, 50))
    out.append(Case("edge-n1", np.array([[2.0]]), np.array([3.0]), np.zeros(1), 50))
    return tuple(out)


def case(small, name):
    return next(c for c in cases(small) if c.name == name)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference loop restated
# ---------------------------------------------------------------------------------------------------------------------------------

LUCKY = ("GMRES has experienced lucky breakdown, but the residual has not converged.\n"
         "                                  Solver terminated without convergence.")
NAN_TEXT = "gmres: Relative residual is nan. Terminating solver."


def restated_gmres(D, b, x0, m, tol, max_restart, ortho, T, M=None):
    """gmres_impl.hpp:59-329 (line numbers in the comments), scalars and vectors in the value type T"""
    with np.errstate(all="ignore"):
        A, B, X = D.astype(T), b.astype(T), x0.astype(T).copy()
        n, one, tol = len(B), T(1), T(tol)
        nrm2 = lambda v: T(np.sqrt(np.dot(v, v)))
        rec = types.SimpleNamespace(short=[], true=[], compared=[], V=None, H=None, last_iters=0, cycles=0, error=None)
        converged, cycle, numIters = False, 0, 0                                     # :79-81
        Xiter = np.zeros(n, T)                                                       # :97
        nrmB = nrm2(B)                                                               # :118
        Res = B.copy()                                                               # :119
        Wj = A @ X                                                                   # :122
        Res = Res - Wj                                                               # :123
        trueRes = nrm2(Res)                                                          # :124
        if nrmB != 0:                                                                # :125-132
            relRes = trueRes / nrmB
        elif trueRes == 0:
            relRes = trueRes
        else:
            X[:] = 0
            relRes = T(0)
        shortRelRes = relRes                                                         # :133
        rec.true.append(float(relRes)); rec.compared.append(float(relRes))
        if relRes < tol:                                                             # :137
            converged = True
        V = np.zeros((n, m + 1), T)
        while (not converged) and cycle <= max_restart and shortRelRes >= 1e-14:      # :141
            GVec = np.zeros(m + 1, T); GVec[0] = trueRes                             # :142
            H = np.zeros((m + 1, m), T); Hraw = np.zeros((m + 1, m), T)
            Cos, Sin = np.zeros(m, T), np.zeros(m, T)
            V[:, 0] = (one / trueRes) * Res                                          # :145-147
            jv = 0
            rec.last_iters = 0
            for j in range(m):                                                       # :149
                Vj = V[:, jv]
                if M is not None:                                                    # :150-155
                    Wj = A @ M(Vj)
                else:
                    Wj = A @ Vj
                if ortho == "MGS":                                                   # :157-163
                    for i in range(j + 1):
                        H[i, j] = np.dot(V[:, i], Wj)
                        Wj = Wj + (-H[i, j]) * V[:, i]
                else:                                                                # :164-178
                    V0j = V[:, :j + 1]
                    Hj = V0j.T @ Wj
                    Wj = Wj - V0j @ Hj
                    tmp = V0j.T @ Wj
                    Wj = Wj - V0j @ tmp
                    H[:j + 1, j] = Hj + tmp
                tmpNrm = nrm2(Wj)                                                    # :183
                H[j + 1, j] = tmpNrm
                Hraw[:, j] = H[:, j]
                if tmpNrm > 1e-14:                                                   # :185-188
                    jv = j + 1
                    V[:, jv] = (one / H[j + 1, j]) * Wj
                for i in range(j):                                                   # :194-198
                    tempVal = Cos[i] * H[i, j] + Sin[i] * H[i + 1, j]
                    H[i + 1, j] = -Sin[i] * H[i, j] + Cos[i] * H[i + 1, j]
                    H[i, j] = tempVal
                f, g = H[j, j], H[j + 1, j]                                          # :199-209
                f2, g2 = f * f, g * g
                fg2 = f2 + g2
                D1 = one / T(np.sqrt(f2 * fg2))
                Cos[j] = f2 * D1
                fg2 = fg2 * D1
                H[j, j] = f * fg2
                Sin[j] = f * D1 * g
                H[j + 1, j] = 0
                GVec[j + 1] = GVec[j] * (-Sin[j])                                    # :211-213
                GVec[j] = GVec[j] * Cos[j]
                shortRelRes = T(abs(GVec[j + 1])) / nrmB
                rec.short.append(float(shortRelRes)); rec.compared.append(float(shortRelRes))
                rec.last_iters = j + 1
                rec.V, rec.H = V, Hraw
                if tmpNrm <= 1e-14 and shortRelRes >= tol:                           # :219-223
                    rec.error = LUCKY
                    return rec
                if np.isnan(shortRelRes):                                            # :224-226
                    rec.error = NAN_TEXT
                    return rec
                if shortRelRes < tol or j == m - 1:                                  # :229
                    y = GVec[:m].copy()                                              # :231-241
                    for i in range(j, -1, -1):
                        s = y[i]
                        for c in range(i + 1, j + 1):
                            s = s - H[i, c] * y[c]
                        y[i] = s / H[i, i]
                    if M is not None:                                                # :249-256
                        Xiter = M(V[:, :j + 1] @ y[:j + 1]) + X
                    else:
                        Xiter = X + V[:, :j + 1] @ y[:j + 1]
                    Wj = A @ Xiter                                                   # :257
                    Res = B - Wj                                                     # :258-259
                    trueRes = nrm2(Res)                                              # :260
                    relRes = trueRes / nrmB                                          # :261
                    rec.true.append(float(relRes)); rec.compared.append(float(relRes))
                    numIters = j + 1                                                 # :265
                    if relRes < tol:                                                 # :267-270
                        converged = True
                        X = Xiter.copy()
                        break
                    elif shortRelRes < 1e-30:                                        # :271-280
                        break
            cycle += 1                                                               # :285
            X = Xiter.copy()                                                         # :289
        rec.flag = "Conv" if converged else ("LOA" if shortRelRes < tol else "NoConv")   # :299-316
        rec.num_iters = (cycle - 1) * m + numIters if cycle > 0 else 0               # :317-321
        rec.cycles, rec.X, rec.end_rel_res = cycle, X, float(relRes)
        return rec


def margin_of(compared, tol):
    vals = [v for v in compared if v > 0 and np.isfinite(v)]
    return min([max(v / tol, tol / v) for v in vals], default=np.inf)


@functools.lru_cache(maxsize=None)
def reference(small, name, dtype, ortho):
    """(tol, the restated run at that tol, its margin) of a case: the target tol when its margin is 1.5, else the middle of the nearest gap of
    2.3 between consecutive short residuals whose run has that margin"""
    c = case(small, name)
    run = lambda tol: restated_gmres(c.D, c.b, c.x0, c.m, tol, c.max_restart, ortho, dtype, c.apply_M(dtype))
    tol = TARGET_TOL[dtype]
    rec = run(tol)
    if margin_of(rec.compared, tol) < 1.5:
        probe = run(tol * 1e-3)                       # the same short residuals (the checks change no state of the loop), further down
        s = [v for v in probe.short if v > 0]
        gaps = sorted((abs(math.log(math.sqrt(a * bb) / tol)), math.sqrt(a * bb)) for a, bb in zip(s, s[1:]) if a / bb >= 2.3)
        for _, cand in gaps[:12]:
            cand = float(dtype(cand))
            if not 1e-3 * tol <= cand <= 1e3 * tol:
                break
            trial = run(cand)
            if margin_of(trial.compared, cand) >= 1.5:
                tol, rec = cand, trial
                break
    return tol, rec, margin_of(rec.compared, tol)


def loss_of_orthogonality(V, ncols):
    Q = V[:, :ncols].astype(LD)
    return float(np.abs(Q.T @ Q - np.eye(ncols, dtype=LD)).max()) if ncols else 0.0


def valid_columns(H, iters):
    """columns of the basis the last cycle wrote: iters + 1 unless the last norm fell under the guard"""
    if iters == 0:
        return 0
    return iters + 1 if H[iters, iters - 1] > 1e-14 else iters


# ---------------------------------------------------------------------------------------------------------------------------------
# running the library
# ---------------------------------------------------------------------------------------------------------------------------------

def make_matrix(kk, be, D, dtype, offset_dtype=np.int32):
    rm, ent, val = dense_to_crs(D)
    return kk.CrsMatrix.from_host(D.shape[0], D.shape[1], rm, ent, val.astype(dtype), offset_dtype=offset_dtype, backend=be)


def make_precond(kk, be, c, dtype, offset_dtype=np.int32, lu_from_spiluk=False):
    """the case's preconditioner on the backend (None when it has none) and what must stay alive with it"""
    if c.precond == "jacobi":
        return kk.MatrixPrec(make_matrix(kk, be, c.Minv, dtype, offset_dtype))
    if c.precond == "lu":
        if lu_from_spiluk:
            return lu_by_spiluk(kk, be, c, dtype, offset_dtype)
        return kk.LUPrec(make_matrix(kk, be, c.L, dtype, offset_dtype), make_matrix(kk, be, c.U, dtype, offset_dtype))
    return None


def lu_by_spiluk(kk, be, c, dtype, offset_dtype=np.int32):
    """ILU(0) by the library's own spiluk, handed to LUPrec"""
    A = make_matrix(kk, be, c.D, dtype, offset_dtype)
    n, nnz = c.n, A.nnz()
    kh = kk.KokkosKernelsHandle(be)
    kh.create_spiluk_handle("SEQLVLSCHD_TP1", n, nnz, nnz)
    Lrm, Urm = be.empty(n + 1, offset_dtype), be.empty(n + 1, offset_dtype)
    Le, Ue = be.empty(nnz + n, np.int32), be.empty(nnz + n, np.int32)
    kk.spiluk_symbolic(kh, 0, A.graph.row_map, A.graph.entries, Lrm, Le, Urm, Ue)
    sh = kh.get_spiluk_handle()
    nl, nu = sh.get_nnzL(), sh.get_nnzU()
    Lv, Uv = be.empty(nnz + n, dtype), be.empty(nnz + n, dtype)
    kk.spiluk_numeric(kh, 0, A.graph.row_map, A.graph.entries, A.values, Lrm, Le, Lv, Urm, Ue, Uv)
    L = kk.CrsMatrix(n, n, Lrm, Le[:nl], Lv[:nl], backend=be)
    U = kk.CrsMatrix(n, n, Urm, Ue[:nu], Uv[:nu], backend=be)
    kh.destroy_spiluk_handle()
    return kk.LUPrec(L, U)


def solve(kk, be, c, dtype, ortho, tol, fuse=1, offset_dtype=np.int32, rows_per_group=0, lu_from_spiluk=False, kh=None, fuse_max_k=64):
    """runs kk.gmres on the case; returns a namespace shaped like restated_gmres's"""
    A = make_matrix(kk, be, c.D, dtype, offset_dtype)
    P = make_precond(kk, be, c, dtype, offset_dtype, lu_from_spiluk)
    own = kh is None
    if own:
        kh = kk.KokkosKernelsHandle(be)
        kh.create_gmres_handle(c.m, tol, c.max_restart)
    gh = kh.get_gmres_handle()
    gh.set_m(c.m); gh.set_tol(tol); gh.set_max_restart(c.max_restart)
    gh.set_ortho(ortho); gh.set("fuse", fuse); gh.set("rows_per_group", rows_per_group); gh.set("fuse_max_k", fuse_max_k)
    B = be.from_numpy(c.b.astype(dtype)); X = be.from_numpy(c.x0.astype(dtype))
    kk.gmres(kh, A, B, X, P)
    r = types.SimpleNamespace(num_iters=gh.get_num_iters(), flag=gh.get_conv_flag_val(), cycles=gh.get("cycles"), end_rel_res=gh.get_end_rel_res(),
                              short=gh.export("short_residuals"), true=gh.export("true_residuals"), H=gh.export("hessenberg"),
                              V=gh.export("basis"), X=np.array(be.to_numpy(X), copy=True), host_syncs=gh.get("host_syncs"),
                              launches=gh.get("launches"), last_fused=gh.get("last_fused"))
    r.compared = [r.true[0]] + list(r.short) + list(r.true[1:])
    r.last_iters = r.num_iters - (r.cycles - 1) * c.m if r.cycles > 0 else 0
    if P is not None:
        P.destroy()
    if own:
        kh.destroy_gmres_handle()
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------------------------------------------------------------

def check_case_shapes(small):
    """conditions on the restated loop alone"""
    for c in cases(small):
        for dtype in DTYPES:
            for ortho in ("CGS2", "MGS"):
                tol, rec, margin = reference(small, c.name, dtype, ortho)
                assert rec.error is None, (c.name, dtype, ortho, rec.error)
                assert margin >= 1.5, (c.name, dtype, ortho, tol, margin)
                assert 1e-3 * TARGET_TOL[dtype] <= tol <= 1e3 * TARGET_TOL[dtype]
                assert rec.flag == "Conv", (c.name, dtype, ortho, rec.flag)
    for dtype in DTYPES:
        for m in (50, 5):
            tol, rec, margin = reference(small, "diag5-m%d" % m, dtype, "CGS2")
            assert rec.num_iters == 5 and rec.cycles == 1 and margin >= (2.8e6 if dtype is np.float64 else 280)
        tol, rec, margin = reference(small, "diag5-m3", dtype, "CGS2")
        assert rec.cycles > 1 and rec.num_iters == (rec.cycles - 1) * 3 + rec.last_iters
        assert reference(small, "tri-lu", dtype, "CGS2")[1].num_iters == 1 and reference(small, "tri-lu", dtype, "CGS2")[2] >= 100
        assert reference(small, "edge-b0", dtype, "CGS2")[1].num_iters == 0 and not reference(small, "edge-b0", dtype, "CGS2")[1].X.any()
        assert reference(small, "edge-x0-solution", dtype, "CGS2")[1].num_iters == 0
        assert reference(small, "edge-n1", dtype, "CGS2")[1].num_iters == 1
        assert reference(small, "conv2d-m4", dtype, "CGS2")[1].cycles > 1
        assert reference(small, "conv2d-m10", dtype, "CGS2")[1].cycles > 1 or small
    plain, lu = reference(small, "conv2d-m50", np.float64, "CGS2")[1], reference(small, "conv2d-lu", np.float64, "CGS2")[1]
    assert lu.num_iters < plain.num_iters
    if not small:
        assert reference(False, "tri", np.float64, "CGS2")[1].num_iters == 13
        assert (lu.num_iters, plain.num_iters) == (12, 38)


def residual_bound(c, x, tol, dtype):
    """Conv means the solver's own evaluation fl(||fl(b - fl(A x))||) / fl(||b||) < tol.  With row length L the evaluated residual differs
    from the true one by at most gamma_{L+1} (|A||x| + |b|) componentwise (L products and L additions per row, one subtraction); each
    norm of n terms carries a relative error of at most gamma_{n+2} (n squares and additions, the root), the quotient one more rounding.
    Hence ||b - A x|| <= tol ||b|| (1 + gamma_{n+2})^2 / (1 - gamma_{n+3}) + gamma_{L+1} || |A||x| + |b| ||."""
    L = int(c.row_len.max())
    A, xl, bl = np.abs(c.D).astype(LD), np.abs(x).astype(LD), np.abs(c.b).astype(LD)
    g = gamma(c.n + 2, dtype)
    return float(tol * np.sqrt((bl * bl).sum()) * (1 + g) ** 2 / (1 - gamma(c.n + 3, dtype)) + gamma(L + 1, dtype) * np.sqrt(((A @ xl + bl) ** 2).sum()))


def check_invariants(c, r, rec, tol, dtype, ortho):
    """item 4: residual of a converged solve, the Arnoldi relation of the last cycle, loss of orthogonality against the restated loop"""
    if r.flag == "Conv":
        x = r.X.astype(LD)
        res = float(np.sqrt(((c.b.astype(LD) - c.D.astype(LD) @ x) ** 2).sum()))
        assert res <= residual_bound(c, r.X, tol, dtype), (c.name, res, residual_bound(c, r.X, tol, dtype))
    k = r.last_iters
    if k == 0:
        return None
    cols = valid_columns(r.H, k)
    V, H = r.V[:, :cols].astype(LD), r.H[:cols, :k].astype(LD)
    A, Md = c.D.astype(LD), c.M_dense().astype(LD)
    L = int(c.row_len.max())
    u = UNIT[dtype]
    # Column j of A M V_k - V_{k+1} H_k, to first order.  z = fl(M v_j) errs by dz: u |z| for the Jacobi product; for the two triangular
    # solves (L + dL) y = v, (U + dU) z = y with |dL| <= gamma_{L+1} |L|, |dU| <= gamma_{L+1} |U| (rows of at most L entries), hence
    # dz <= gamma_{L+1} (|U^-1||U||z| + |U^-1||L^-1||L||y|).  fl(A z) errs by gamma_L |A|(|z| + dz) and carries |A| dz.  The two
    # projections w - V h each err by gamma_{k+2} (|w| + |V||h|) with |w| <= |A||z| and |h1|, |h2| <= 2 |h| entrywise to first order;
    # h = h1 + h2 and the scaling by 1 / nrm add 3 u (|V||h| + nrm |v_{j+1}|), both inside |V_{k+1}||H(:,j)|.
    if c.precond == "lu":
        Linv, Uinv = np.abs(np.linalg.inv(c.L)).astype(LD), np.abs(np.linalg.inv(c.U)).astype(LD)
        Ll, Ul = np.abs(c.L).astype(LD), np.abs(c.U).astype(LD)
        Lsolve = np.linalg.inv(c.L).astype(LD)
    for j in range(k):
        z = np.abs(Md @ V[:, j])
        if c.precond == "lu":
            dz = gamma(L + 1, dtype) * (Uinv @ (Ul @ z) + Uinv @ (Linv @ (Ll @ np.abs(Lsolve @ V[:, j]))))
        elif c.precond == "jacobi":
            dz = u * z
        else:
            dz = 0 * z
        Az = np.abs(A) @ z
        Vh = np.abs(V) @ np.abs(H[:, j])
        bound = np.abs(A) @ dz + gamma(L, dtype) * (np.abs(A) @ (z + dz)) + 2 * gamma(k + 2, dtype) * (Az + 2 * Vh) + 3 * u * Vh
        lhs = A @ (Md @ V[:, j]) - V @ H[:, j]
        assert float(np.sqrt((lhs ** 2).sum())) <= float(np.sqrt((bound ** 2).sum())), (c.name, j, float(np.abs(lhs).max()), float(bound.max()))
    if ortho == "CGS2":
        loo = loss_of_orthogonality(r.V, cols)
        ref = loss_of_orthogonality(rec.V, valid_columns(rec.H, rec.last_iters)) if rec.V is not None else 0.0
        limit = 8 * max(ref, gamma(c.n, dtype))
        assert loo <= limit, (c.name, loo, ref, limit)
        return loo / max(ref, gamma(c.n, dtype))
    return None


def check_solver(kk, be, small, name, dtype, ortho, fuse=1, offset_dtype=np.int32, rows_per_group=0, lu_from_spiluk=False):
    """items 3 and 4 for one case"""
    c = case(small, name)
    tol, rec, margin = reference(small, name, dtype, ortho)
    r = solve(kk, be, c, dtype, ortho, tol, fuse, offset_dtype, rows_per_group, lu_from_spiluk)
    print("%s %s %s fuse=%d: iters %d (restated %d) flag %s cycles %d margin %.3g tol %.3g" % (name, np.dtype(dtype).name, ortho, fuse, r.num_iters,
                                                                                            rec.num_iters, r.flag, r.cycles, margin, tol))
    single = rec.cycles <= 1
    if dtype is np.float64 or margin >= 100:
        assert margin >= 1.5
        assert (r.num_iters, r.flag, r.cycles) == (rec.num_iters, rec.flag, rec.cycles), (name, r.num_iters, rec.num_iters, r.flag, rec.flag)
    elif single:
        assert abs(r.num_iters - rec.num_iters) <= 1 and r.flag == rec.flag, (name, r.num_iters, rec.num_iters, r.flag)
    if r.cycles > 0:
        assert r.num_iters == (r.cycles - 1) * c.m + r.last_iters and 1 <= r.last_iters <= c.m
        assert len(r.short) == r.num_iters
    assert r.flag in ("Conv", "NoConv", "LOA")
    assert abs(r.end_rel_res - r.true[-1]) <= 1e-6 * abs(r.true[-1])      # end_rel_res is the last relRes, a value of the value type held as double
    if ortho == "CGS2":
        assert r.host_syncs == 1 + r.num_iters + (len(r.true) - 1), (r.host_syncs, r.num_iters, len(r.true))
    ratio = check_invariants(c, r, rec, tol, dtype, ortho)
    return r, ratio


# kernels ---------------------------------------------------------------------------------------------------------------------------

KERNEL_N = (1, 63, 64, 65, 1000, 4097)
KERNEL_K = (1, 2, 7, 8, 9, 16, 17, 50, 64, 65)


def kernel_bits(n, k, dtype):
    p = PBITS[dtype]
    return min((p - 1 - math.ceil(math.log2(n)) if n > 1 else p - 1) // 2, (p - 3 - math.ceil(math.log2(k)) if k > 1 else p - 3) // 2, 12)


def kernel_data(n, k, ldv, alpha, dtype, seed):
    b = kernel_bits(n, k, dtype)
    assert b >= (8 if dtype is np.float64 else 3), (n, k, b)
    rng = np.random.default_rng(seed)
    draw = lambda *shape: rng.integers(-(2 ** b) + 1, 2 ** b, size=shape).astype(np.float64) / 16
    V = np.zeros((ldv, k)); V[:n] = draw(n, k); V[n:] = np.nan          # the padding rows of V are never read
    h, w, d = draw(k), draw(n), draw(n)
    w_in = d - alpha * (V[:n] @ h)
    for a in (V[:n], h, w, d, w_in):
        assert np.array_equal(a.astype(dtype).astype(np.float64), a)
    return V, h, w, d, w_in


class Blocks:
    """kkamd_gmres_dot / kkamd_gmres_update on backend arrays"""

    def __init__(self, kk, be, rows_per_group=0, fuse=1):
        self.kk, self.be = kk, be
        self.kh = kk.KokkosKernelsHandle(be)
        self.kh.create_gmres_handle()
        self.gh = self.kh.get_gmres_handle()
        self.gh.set("rows_per_group", rows_per_group); self.gh.set("fuse", fuse); self.gh.set("fuse_max_k", 64)   # the kernel at every k it takes

    def dot(self, V, n, k, ldv, w, dtype):
        be, lib = self.be, self.be.lib
        dV, dw, dh = be.from_numpy(V.T.reshape(-1).astype(dtype)), be.from_numpy(w.astype(dtype)), be.empty(k, dtype)
        self.kk._capi.check(lib, lib.kkamd_gmres_dot(self.gh.h, n, k, be.ptr(dV), ldv, be.ptr(dw), be.ptr(dh), self.kk._capi.F64 if dtype is np.float64 else self.kk._capi.F32, be.stream()))
        return np.array(be.to_numpy(dh), copy=True)

    def update(self, V, n, k, ldv, alpha, h, w_in, dtype, alias=False, want_h2=True, want_ss=True):
        be, lib = self.be, self.be.lib
        dV, dh = be.from_numpy(V.T.reshape(-1).astype(dtype)), be.from_numpy(h.astype(dtype))
        dwi = None if w_in is None else be.from_numpy(w_in.astype(dtype))
        dwo = dwi if alias else be.from_numpy(np.full(n, 77.0, dtype))
        dh2 = be.from_numpy(np.full(k, 77.0, dtype)) if want_h2 else None
        dss = be.from_numpy(np.full(1, 77.0, dtype)) if want_ss else None
        self.kk._capi.check(lib, lib.kkamd_gmres_update(self.gh.h, n, k, float(alpha), be.ptr(dV), ldv, be.ptr(dh), be.ptr(dwi), be.ptr(dwo), be.ptr(dh2),
                                                      be.ptr(dss), self.kk._capi.F64 if dtype is np.float64 else self.kk._capi.F32, be.stream()))
        get = lambda a: None if a is None else np.array(be.to_numpy(a), copy=True)
        return get(dwo), get(dh2), get(dss), self.gh.get("last_fused")

    def close(self):
        self.kh.destroy_gmres_handle()


def check_kernels_exact(kk, be, n, k, dtype, seed=0, pick=(0, 1, 2, 3)):
    """item 1: dot, update, fused second product and sum of squares against numpy in longdouble, ==, over ldv, rows_per_group, aliasing, alpha"""
    combos = [(n, 0, False, -1.0, 1), (n + 3, 64, True, 1.0, 1), (n + 3, 0, False, 2.0, 0), (n, 64, True, -1.0, 0)]
    for ldv, rpg, alias, alpha, fuse in [combos[i] for i in pick]:
        V, h, w, d, w_in = kernel_data(n, k, ldv, alpha, dtype, seed + 13 * n + k)
        blk = Blocks(kk, be, rpg, fuse)
        Vl = V[:n].astype(LD)
        got = blk.dot(V, n, k, ldv, w, dtype)
        assert np.array_equal(got.astype(LD), Vl.T @ w.astype(LD)), ("dot", n, k, ldv, rpg)
        wo, h2, ss, fused = blk.update(V, n, k, ldv, alpha, h, w_in, dtype, alias)
        assert fused == (1 if fuse and k <= blk.gh.get("fuse_max_k") else 0), (n, k, fuse, fused)
        assert np.array_equal(wo.astype(LD), d.astype(LD)), ("update", n, k, ldv, rpg, alpha)
        assert np.array_equal(h2.astype(LD), Vl.T @ d.astype(LD)), ("second product", n, k, ldv, rpg, fuse)
        assert np.array_equal(ss.astype(LD), [(d.astype(LD) ** 2).sum()]), ("sum of squares", n, k)
        wo2, h2n, ssn, fused = blk.update(V, n, k, ldv, alpha, h, None, dtype, False, want_h2=False, want_ss=False)   # w_in NULL: alpha V h
        assert fused == 0 and h2n is None and ssn is None
        assert np.array_equal(wo2.astype(LD), alpha * (Vl @ h.astype(LD)))
        blk.close()


def check_kernels_nonfinite(kk, be, dtype, fuse):
    """Inf / NaN in one entry of w reach exactly the outputs they should"""
    n, k, ldv = 300, 9, 303
    V, h, w, d, w_in = kernel_data(n, k, ldv, -1.0, dtype, 5)
    V[17, 3] = 0.0
    w_in = d + (V[:n] @ h)
    blk = Blocks(kk, be, 64, fuse)
    with np.errstate(all="ignore"):
        for bad in (np.inf, -np.inf, np.nan):
            w2 = w.copy(); w2[17] = bad
            got = blk.dot(V, n, k, ldv, w2, dtype)
            exp = (V[:n].T @ w).astype(dtype) + np.array([np.nan if V[17, c] == 0 or np.isnan(bad) else np.sign(V[17, c]) * bad for c in range(k)])
            assert np.array_equal(got, exp.astype(dtype), equal_nan=True), (bad, got, exp)
            wi = w_in.copy(); wi[17] = bad
            wo, h2, ss, _ = blk.update(V, n, k, ldv, -1.0, h, wi, dtype)
            dd = d.copy(); dd[17] = bad
            assert np.array_equal(wo, dd.astype(dtype), equal_nan=True)
            exp2 = (V[:n].T @ d) + np.array([np.nan if V[17, c] == 0 or np.isnan(bad) else np.sign(V[17, c]) * bad for c in range(k)])
            assert np.array_equal(h2, exp2.astype(dtype), equal_nan=True), (bad, h2, exp2)
            assert (np.isnan(ss[0]) if np.isnan(bad) else ss[0] == np.inf)
    blk.close()


def check_fuse_equivalence(kk, be, n, k, dtype, runs=(0, 1, 0, 1)):
    """item 2: on rounded random values fuse 0 and fuse 1 give the same bits, and so do two runs of either"""
    rng = np.random.default_rng(n + k)
    V = rng.uniform(-1, 1, (n + 3, k)).astype(dtype); h = rng.uniform(-1, 1, k).astype(dtype); w = rng.uniform(-1, 1, n).astype(dtype)
    outs = []
    for fuse in runs:
        blk = Blocks(kk, be, 64 if n < 2000 else 0, fuse)
        h1 = blk.dot(V, n, k, n + 3, w, dtype)
        wo, h2, ss, fused = blk.update(V, n, k, n + 3, -1.0, h1, w, dtype)
        assert fused == (1 if fuse and k <= 64 else 0)
        outs.append((h1, wo, h2, ss))
        blk.close()
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert a.tobytes() == b.tobytes()
    # and the result is the projection to rounding: |V^T w'| small against |V||w|
    assert np.isfinite(outs[0][1]).all()


# preconditioners -------------------------------------------------------------------------------------------------------------------

def check_preconditioners(kk, be, small, dtype, lu_from_spiluk=False):
    """item 5: apply with (alpha, beta) in {(1,0), (1,1), (2,-1)} for the three kinds against numpy; the callback kind calling kkamd_spmv
    reproduces the matrix kind's bits"""
    u = UNIT[dtype]
    rng = np.random.default_rng(3)
    for name in ("conv2d-jacobi", "conv2d-lu", "tri-lu"):
        c = case(small, name)
        P = make_precond(kk, be, c, dtype, lu_from_spiluk=lu_from_spiluk)
        Md = c.M_dense().astype(LD)
        x = rng.uniform(-1, 1, c.n).astype(dtype); y0 = rng.uniform(-1, 1, c.n).astype(dtype)
        for alpha, beta in ((1.0, 0.0), (1.0, 1.0), (2.0, -1.0)):
            ystart = y0.copy()
            if beta == 0.0:
                ystart[::7] = np.nan                              # beta == 0 does not read y
            Y = be.from_numpy(ystart)
            P.apply(be.from_numpy(x), Y, "N", alpha, beta)
            got = np.array(be.to_numpy(Y), copy=True).astype(LD)
            exp = alpha * (Md @ x.astype(LD)) + (beta * y0.astype(LD) if beta != 0.0 else 0)
            # forward error of the product / of the two solves: gamma_n cond-weighted, |M| |x| with |U^-1||L^-1| for the factors
            absM = np.abs(Md) if c.precond == "jacobi" else np.abs(np.linalg.inv(c.U)).astype(LD) @ np.abs(np.linalg.inv(c.L)).astype(LD)
            amp = 1 if c.precond == "jacobi" else float((np.abs(c.L) @ np.abs(c.U)).sum(axis=1).max())
            bound = abs(alpha) * gamma(2 * c.n, dtype) * amp * (absM @ np.abs(x).astype(LD)) + 3 * u * (np.abs(exp) + np.abs(y0))
            assert (np.abs(got - exp) <= bound).all(), (name, alpha, beta, float(np.abs(got - exp).max()), float(bound.min()))
        P.destroy()
    # callback == matrix kind, bit for bit
    c = case(small, "conv2d-jacobi")
    Mm = make_matrix(kk, be, c.Minv, dtype)
    P = kk.MatrixPrec(Mm)

    class Foreign(kk.Preconditioner):
        def __init__(self):
            super().__init__(be)
            self.d = Mm.desc()
            self.calls = 0
            self._init_callback()

        def apply_device(self, d_x, d_y, alpha, beta, value_type, stream):
            self.calls += 1
            return be.lib.kkamd_spmv(None, C.byref(self.d), b"N", alpha, d_x, beta, d_y, value_type, stream)
    F = Foreign()
    x = rng.uniform(-1, 1, c.n).astype(dtype); y0 = rng.uniform(-1, 1, c.n).astype(dtype)
    Pn = kk.MatrixPrec(Mm)
    for alpha, beta in ((1.0, 0.0), (1.0, 1.0), (2.0, -1.0)):
        Y1, Y2 = be.from_numpy(y0.copy()), be.from_numpy(y0.copy())
        P.apply(be.from_numpy(x), Y1, "N", alpha, beta)
        F.apply(be.from_numpy(x), Y2, "N", alpha, beta)
        a, b2 = np.array(be.to_numpy(Y1)), np.array(be.to_numpy(Y2))
        assert np.array_equal(a, b2), (alpha, beta)
    assert F.calls == 3
    # and GMRES with the foreign preconditioner takes the steps it takes with the matrix kind
    tol, rec, margin = reference(small, "conv2d-jacobi", dtype, "CGS2")
    res = []
    for prec in (Pn, F):
        kh = kk.KokkosKernelsHandle(be)
        kh.create_gmres_handle(c.m, tol, c.max_restart)
        X = be.from_numpy(c.x0.astype(dtype))
        kk.gmres(kh, make_matrix(kk, be, c.D, dtype), be.from_numpy(c.b.astype(dtype)), X, prec)
        res.append((kh.get_gmres_handle().get_num_iters(), np.array(be.to_numpy(X), copy=True)))
        kh.destroy_gmres_handle()
    assert res[0][0] == res[1][0] and np.allclose(res[0][1], res[1][1], rtol=0, atol=1e3 * UNIT[dtype])
    for q in (P, Pn, F):
        q.destroy()


# errors and state ------------------------------------------------------------------------------------------------------------------

def check_errors_and_state(kk, be, small):
    """item 6"""
    cap = kk._capi
    lib = be.lib
    c = case(small, "conv2d-m50")
    # m <= 0, with the reference's text
    with pytest.raises(ValueError, match="Please choose restart size m greater than zero"):
        kk.KokkosKernelsHandle(be).create_gmres_handle(0)
    kh = kk.KokkosKernelsHandle(be)
    with pytest.raises(ValueError, match="does not have an GMRES handle"):
        kk.gmres(kh, None, None, None)
    kh.create_gmres_handle()
    gh = kh.get_gmres_handle()
    assert (gh.get_m(), gh.get_tol(), gh.get_max_restart(), gh.get_ortho(), gh.get_verbose()) == (50, 1e-8, 50, "CGS2", False)
    assert (gh.get("fuse"), gh.get("fuse_max_k"), gh.get("rows_per_group")) == (1, 17, 0)
    with pytest.raises(cap.KkamdError):
        gh.set("fuse_max_k", 65)
    assert gh.get_conv_flag_val() == "NotRun" and gh.get("num_iters") == -1 and gh.get_real("end_rel_res") == -1
    with pytest.raises(AssertionError):
        gh.get_num_iters()
    with pytest.raises(cap.KkamdError) as e:
        gh.set("m", 0)
    assert e.value.status == cap.ERR_INVALID_ARG
    with pytest.raises(cap.KkamdError):
        gh.set("no_such_knob", 1)
    with pytest.raises(cap.KkamdError):
        gh.set("rows_per_group", 100)
    with pytest.raises(ValueError):
        gh.set_ortho("CGS")
    # dimension mismatch: the reference's text
    A = make_matrix(kk, be, c.D, np.float64)
    B = be.from_numpy(c.b); Xs = be.from_numpy(np.zeros(c.n + 1))
    with pytest.raises(RuntimeError, match="KokkosSparse::gmres: Dimensions do not match: , A: %d x %d, x: %d, b: %d" % (c.n, c.n, c.n + 1, c.n)):
        kk.gmres(kh, A, B, Xs)
    R = kk.CrsMatrix.from_host(c.n, c.n + 1, c.row_map, c.entries, c.values, backend=be)
    d = R.desc()
    assert lib.kkamd_gmres_solve(gh.h, C.byref(d), be.ptr(B), be.ptr(Xs), None, cap.F64, be.stream()) == cap.ERR_INVALID_ARG
    assert b"KokkosSparse::gmres: Dimensions do not match: , A: %d x %d, x: %d, b: %d" % (c.n, c.n + 1, c.n + 1, c.n) in lib.kkamd_last_error()
    # type pairs
    d = A.desc()
    X = be.from_numpy(np.zeros(c.n))
    assert lib.kkamd_gmres_solve(gh.h, C.byref(d), be.ptr(B), be.ptr(X), None, cap.F32, be.stream()) == cap.ERR_UNSUPPORTED
    assert lib.kkamd_gmres_solve(gh.h, C.byref(d), be.ptr(B), be.ptr(X), None, 5, be.stream()) == cap.ERR_UNSUPPORTED
    assert gh.get_conv_flag_val() == "NotRun"
    # NaN in b
    bn = c.b.copy(); bn[3] = np.nan
    with pytest.raises(RuntimeError, match="gmres: Relative residual is nan. Terminating solver."):
        kk.gmres(kh, A, be.from_numpy(bn), X)
    assert lib.kkamd_gmres_solve(gh.h, C.byref(d), be.ptr(be.from_numpy(bn)), be.ptr(X), None, cap.F64, be.stream()) == cap.ERR_NUMERIC
    # lucky breakdown without convergence: n = 1, A = 2, b = 3 and tol = 0: the first iteration leaves w = 0 exactly and shortRelRes = 0 >= tol.
    # (With tol > 0 the branch needs |sin| >= tol from a norm under 1e-14, out of reach for the tolerances of the cases.)
    # A = diag(1, 1, 0, 0), b = 1: every value is exact, the second iteration leaves w = 0 and a zero pivot: the NaN text from inside the loop
    for dtype in DTYPES:
        S1 = kk.CrsMatrix.from_host(1, 1, [0, 1], [0], np.array([2], dtype), backend=be)
        S4 = kk.CrsMatrix.from_host(4, 4, [0, 1, 2, 3, 4], [0, 1, 2, 3], np.array([1, 1, 0, 0], dtype), backend=be)
        for ortho in ("CGS2", "MGS"):
            gh.set_ortho(ortho)
            gh.set_tol(0.0)
            with pytest.raises(RuntimeError, match="GMRES has experienced lucky breakdown, but the residual has not converged."):
                kk.gmres(kh, S1, be.from_numpy(np.array([3], dtype)), be.from_numpy(np.zeros(1, dtype)))
            assert restated_gmres(np.array([[2.0]]), np.array([3.0]), np.zeros(1), 50, 0.0, 50, ortho, dtype).error == LUCKY
            gh.set_tol(TARGET_TOL[dtype])
            with pytest.raises(RuntimeError, match=NAN_TEXT):
                kk.gmres(kh, S4, be.from_numpy(np.ones(4, dtype)), be.from_numpy(np.zeros(4, dtype)))
            assert gh.get("num_short_residuals") == 2
            rec = restated_gmres(np.diag([1.0, 1, 0, 0]), np.ones(4), np.zeros(4), 50, TARGET_TOL[dtype], 50, ortho, dtype)
            assert rec.error == NAN_TEXT and len(rec.short) == 2
    # the handle is reused with another n and type, and reset
    gh.reset_handle()
    assert gh.get_conv_flag_val() == "NotRun" and gh.get_ortho() == "CGS2"
    seen = []
    for name, dtype in (("conv2d-m50", np.float64), ("tri", np.float64), ("tri", np.float32), ("edge-n1", np.float64), ("conv2d-m50", np.float64)):
        cc = case(small, name)
        tol, rec, margin = reference(small, name, dtype, "CGS2")
        r = solve(kk, be, cc, dtype, "CGS2", tol, kh=kh)
        assert (r.num_iters, r.flag) == (rec.num_iters, rec.flag) or dtype is np.float32
        assert gh.get("num_rows") == cc.n and gh.get("plan_bytes") >= cc.n * (cc.m + 5) * np.dtype(dtype).itemsize
        seen.append(r.X)
    assert np.array_equal(seen[0], seen[-1])                       # the same bits after the workspace went through other sizes
    # verbose prints the reference's lines (stdout of the library; not captured here) and changes nothing
    kh.destroy_gmres_handle()
    assert kh.get_gmres_handle() is None
