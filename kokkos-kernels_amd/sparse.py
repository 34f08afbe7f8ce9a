"""Thin, reference-shaped front end over the C ABI (names follow KokkosSparse: CrsMatrix with
graph.row_map / graph.entries / values, SPMVHandle, KokkosKernelsHandle + spgemm_symbolic/numeric).

Arrays live wherever the Backend puts them: `torch_backend()` = HBM tensors on the current CUDA/HIP
device (the product path).  tests/emu provides a numpy Backend bound to the emulator build for
logic tests on machines without a GPU; nothing in this file computes anything itself.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import F32, F64, I32, I64, CrsDesc, check


class Backend:
    """How arrays are allocated and how their device pointer / stream are obtained."""

    def __init__(self, lib, empty, ptr, stream, to_numpy, from_numpy, name):
        self.lib, self.empty, self.ptr, self.stream = lib, empty, ptr, stream
        self.to_numpy, self.from_numpy, self.name = to_numpy, from_numpy, name


_TORCH_BACKEND = None


def torch_backend():
    global _TORCH_BACKEND
    if _TORCH_BACKEND is None:
        import torch                     # (before the library is loaded: see lib() on the load order)
        from . import lib, device_check
        if torch.cuda.is_available():
            device_check()               # the library's own runtime must see the device too (it does not when it was loaded before torch)
        if not torch.cuda.is_available():
            raise RuntimeError("kokkos-kernels_amd needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU path")
        tdt = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32,
               np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64}

        def empty(n, dtype):
            return torch.empty(int(n), dtype=tdt[np.dtype(dtype)], device="cuda")

        def from_numpy(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")

        _TORCH_BACKEND = Backend(lib(), empty, lambda t: None if t is None else t.data_ptr(),
                                 lambda: torch.cuda.current_stream().cuda_stream,
                                 lambda t: t.detach().cpu().numpy(), from_numpy, "torch")
    return _TORCH_BACKEND


def _np_dtype(a):
    s = str(a.dtype).replace("torch.", "")
    return np.dtype(s)


def _scalar_type(a):
    return {np.dtype(np.float32): F32, np.dtype(np.float64): F64}[_np_dtype(a)]


def _offset_type(a):
    return {np.dtype(np.int32): I32, np.dtype(np.int64): I64}[_np_dtype(a)]


class _Graph:
    def __init__(self, row_map, entries):
        self.row_map, self.entries = row_map, entries


class CrsMatrix:
    """KokkosSparse::CrsMatrix as the hot path sees it (sparse/src/KokkosSparse_CrsMatrix.hpp:317-388):
    graph.row_map (offset[numRows+1]), graph.entries (int32[nnz]), values (scalar[nnz]), numCols."""

    def __init__(self, num_rows, num_cols, row_map, entries, values, backend=None):
        self.backend = backend or torch_backend()
        self._nrows, self._ncols = int(num_rows), int(num_cols)
        self.graph = _Graph(row_map, entries)
        self.values = values
        self._nnz = int(entries.shape[0]) if entries is not None else 0

    @classmethod
    def from_host(cls, num_rows, num_cols, row_map, entries, values, offset_dtype=np.int32, backend=None):
        be = backend or torch_backend()
        return cls(num_rows, num_cols, be.from_numpy(np.asarray(row_map).astype(offset_dtype)),
                   be.from_numpy(np.asarray(entries).astype(np.int32)),
                   None if values is None else be.from_numpy(np.asarray(values)), backend=be)

    def numRows(self): return self._nrows
    def numCols(self): return self._ncols
    def nnz(self): return self._nnz

    def desc(self):
        be = self.backend
        d = CrsDesc()
        d.num_rows, d.num_cols, d.nnz = self._nrows, self._ncols, self._nnz
        d.d_row_map = be.ptr(self.graph.row_map)
        d.d_entries = be.ptr(self.graph.entries) if self._nnz else None
        d.d_values = be.ptr(self.values) if (self._nnz and self.values is not None) else None
        d.offset_type = _offset_type(self.graph.row_map)
        d.value_type = _scalar_type(self.values) if self.values is not None else F64
        return d

    def to_host(self):
        be = self.backend
        return (be.to_numpy(self.graph.row_map), be.to_numpy(self.graph.entries),
                None if self.values is None else be.to_numpy(self.values))


_ALGOS = {"SPMV_DEFAULT": 0, "SPMV_FAST_SETUP": 1, "SPMV_NATIVE": 2, "SPMV_MERGE_PATH": 3, "SPMV_NATIVE_MERGE_PATH": 4}


class SPMVHandle:
    """KokkosSparse::SPMVHandle (sparse/src/KokkosSparse_spmv_handle.hpp:280-349): carries the algorithm
    choice; the per-matrix plan is created lazily by the first spmv call and freed with the handle."""

    def __init__(self, algo="SPMV_DEFAULT", backend=None):
        if algo not in _ALGOS:
            raise ValueError("SPMVHandle: algorithm %s cannot be used if A is a CrsMatrix" % algo)
        self.algo = algo
        self.backend = backend
        self._plan = None
        self._pending = {}

    def get_algorithm(self): return self.algo

    def set(self, key, value):
        """expert knobs (the reference exposes team_size / vector_length / ... as public members)"""
        if self._plan is None:
            self._pending[key] = value
        else:
            check(self.backend.lib, self.backend.lib.kkamd_spmv_plan_set(self._plan, key.encode(), int(value)))

    def values_changed(self):
        """the caller wrote to A.values: re-ordered copies the plan keeps (cached transpose, column-slab copy) copy them again at the next
        call (kkamd_spmv_plan_values_changed; required under the knob values_tracking = 1, optional otherwise)"""
        if self._plan is not None:
            check(self.backend.lib, self.backend.lib.kkamd_spmv_plan_values_changed(self._plan))

    def query(self, key):
        """what the analysis produced (kkamd_spmv_plan_query); None before the first spmv call"""
        if self._plan is None: return None
        v = C.c_int64(0)
        check(self.backend.lib, self.backend.lib.kkamd_spmv_plan_query(self._plan, key.encode(), C.byref(v)))
        return int(v.value)

    def export(self, what, count):
        """a per-tile array of the analysis ("tile_first_row", "tile_mode") as a host int32 array"""
        out = np.zeros(int(count), dtype=np.int32)
        check(self.backend.lib, self.backend.lib.kkamd_spmv_plan_export(self._plan, what.encode(), out.ctypes.data_as(C.c_void_p), int(count)))
        return out

    def _ensure(self, A, rank2=False):
        if self._plan is None:
            if rank2 and "defer_rank1" not in self._pending:
                # the reference's handle is set up by its first spmv call, for that call's rank (spmv_handle.hpp:280-349): a handle that
                # begins with rank 2 leaves the rank-1 analysis to the first rank-1 call, if one ever comes
                self._pending["defer_rank1"] = 1
            self.backend = A.backend
            lib = A.backend.lib
            p = C.c_void_p()
            d = A.desc()
            n = len(self._pending)                 # the handle's knobs go in with the creation: they shape the analysis
            keys = (C.c_char_p * max(n, 1))(*[k.encode() for k in self._pending])
            vals = (C.c_int * max(n, 1))(*[int(v) for v in self._pending.values()])
            check(lib, lib.kkamd_spmv_plan_create_knobs(C.byref(p), C.byref(d), _ALGOS[self.algo], keys, vals, n, A.backend.stream()))
            self._plan = p
        return self._plan

    def __del__(self):
        try:
            if self._plan is not None and self.backend is not None:
                self.backend.lib.kkamd_spmv_plan_destroy(self._plan)
        except Exception:
            pass
        self._plan = None


def _strides(a):
    if hasattr(a, "stride") and callable(a.stride):
        return tuple(a.stride())
    return tuple(s // a.itemsize for s in a.strides)


def _vec_stride(v, who):
    """element stride of a rank-1 vector; 1 for a vector of at most one element (its stride is never used).  The C ABI
    takes positive strides only: a reversed (negative) or broadcast (zero) view is refused here"""
    if v.shape[0] <= 1:
        return 1
    s = _strides(v)[0]
    if s <= 0:
        raise RuntimeError("KokkosSparse::%s: vector stride %d is not supported (positive strides only)" % (who, s))
    return s


def spmv(*args):
    """KokkosSparse::spmv.  spmv(mode, alpha, A, x, beta, y) or spmv(handle, mode, alpha, A, x, beta, y)
    (the execution-space overloads map to the backend's current stream).  x, y rank 1 or rank 2.
    Dimension checks and messages follow sparse/src/KokkosSparse_spmv.hpp:126-142."""
    if isinstance(args[0], SPMVHandle):
        handle, mode, alpha, A, x, beta, y = args
    else:
        handle = None
        mode, alpha, A, x, beta, y = args
    be, lib = A.backend, A.backend.lib
    if len(x.shape) != len(y.shape) or len(x.shape) not in (1, 2):
        raise RuntimeError("KokkosSparse::spmv: Vector ranks do not match.")
    m, n = A.numRows(), A.numCols()
    xr, yr = x.shape[0], y.shape[0]
    xc = x.shape[1] if len(x.shape) == 2 else 1
    yc = y.shape[1] if len(y.shape) == 2 else 1
    trans = mode[0] in "TtHh"
    if mode[0] not in "NnCcTtHh":
        raise RuntimeError("Invalid transpose mode %s for KokkosSparse::spmv()" % mode)
    if xc != yc or (not trans and (n != xr or m != yr)) or (trans and (m != xr or n != yr)):
        raise RuntimeError("KokkosSparse::spmv: Dimensions do not match%s: , A: %d x %d, x: %d x %d, y: %d x %d"
                           % (" (transpose)" if trans else "", m, n, xr, xc, yr, yc))
    plan = handle._ensure(A, rank2=(len(x.shape) == 2 and xc > 1)) if handle is not None else None
    d = A.desc()
    vt = _scalar_type(y)
    if len(x.shape) == 1:
        xs, ys = _vec_stride(x, "spmv"), _vec_stride(y, "spmv")
        if xs == 1 and ys == 1:
            check(lib, lib.kkamd_spmv(plan, C.byref(d), mode[0].encode(), float(alpha), be.ptr(x), float(beta), be.ptr(y),
                                      vt, be.stream()))
        else:
            # a strided rank-1 view (a column of a row-major multivector, a slice with a step): one column of the rank-2
            # path, in place (as host/KokkosSparse_spmv.hpp does for strided Kokkos views)
            check(lib, lib.kkamd_spmv_mv(plan, C.byref(d), mode[0].encode(), float(alpha), be.ptr(x), xs, xr,
                                         float(beta), be.ptr(y), ys, yr, 1, vt, be.stream()))
    else:
        xs, ys = _strides(x), _strides(y)
        check(lib, lib.kkamd_spmv_mv(plan, C.byref(d), mode[0].encode(), float(alpha), be.ptr(x), xs[0], xs[1],
                                     float(beta), be.ptr(y), ys[0], ys[1], xc, vt, be.stream()))
    return y


def spmv_struct(mode, stencil_type, structure, alpha, A, x, beta, y):
    """KokkosSparse::Experimental::spmv_struct (sparse/src/KokkosSparse_spmv.hpp:478-848).  structure: the grid extents
    (ni[, nj[, nk]]) as a host sequence; stencil_type 1 = FD (3/5/7-pt), 2 = FE (3/9/27-pt).  Rank-2 x/y with one
    column take the structured path, more columns fall through to spmv (:803-831)."""
    be, lib = A.backend, A.backend.lib
    if len(x.shape) != len(y.shape) or len(x.shape) not in (1, 2):
        raise RuntimeError("KokkosSparse::spmv_struct: Vector ranks do not match.")
    m, n = A.numRows(), A.numCols()
    xr, yr = x.shape[0], y.shape[0]
    xc = x.shape[1] if len(x.shape) == 2 else 1
    yc = y.shape[1] if len(y.shape) == 2 else 1
    if mode[0] not in "NnCcTtHh":
        raise RuntimeError("Invalid transpose mode %s for KokkosSparse::spmv_struct()" % mode)
    trans = mode[0] in "TtHh"
    # the reference only requires the vectors to be long enough here (:504-523)
    if xc != yc or (not trans and (n > xr or m > yr)) or (trans and (n > yr or m > xr)):
        raise RuntimeError("KokkosSparse::spmv_struct: Dimensions do not match%s: , A: %d x %d, x: %d x %d, y: %d x %d"
                           % (" (transpose)" if trans else "", m, n, xr, xc, yr, yc))
    if len(x.shape) == 2:
        if xc != 1:
            return spmv(mode, alpha, A, x, beta, y)
        xs, ys = _strides(x), _strides(y)
        strided = xs[0] != 1 or ys[0] != 1
    else:
        strided = _vec_stride(x, "spmv_struct") != 1 or _vec_stride(y, "spmv_struct") != 1
    if strided:
        # strided vectors take the unstructured path, on their leading numCols / numRows elements (they may be longer)
        nin, nout = (m, n) if trans else (n, m)
        spmv(mode, alpha, A, x[:nin], beta, y[:nout])
        return y
    st =(C.c_int64 * len(structure))(*[int(v) for v in structure])
    d = A.desc()
    check(lib, lib.kkamd_spmv_struct(C.byref(d), mode[0].encode(), int(stencil_type), len(structure), st, float(alpha),
                                     be.ptr(x), float(beta), be.ptr(y), _scalar_type(y), be.stream()))
    return y


class _SpgemmHandle:
    def __init__(self, backend):
        self.backend = backend
        self.h = C.c_void_p()
        check(backend.lib, backend.lib.kkamd_spgemm_create(C.byref(self.h)))

    def get(self, what):
        v = C.c_int64()
        check(self.backend.lib, self.backend.lib.kkamd_spgemm_get(self.h, what, C.byref(v)))
        return int(v.value)

    def set(self, key, value):
        """SPGEMMHandle / KokkosKernelsHandle option setters (kkamd_spgemm_set): "algorithm", "accumulator", "compression",
        "compression_cut_off", "verbose" act; the reference's team / shared-memory / hash-scale hints are accepted and recorded
        (get_hint), without effect; unknown keys raise KkamdError(INVALID_ARG)"""
        check(self.backend.lib, self.backend.lib.kkamd_spgemm_set(self.h, key.encode(), float(value)))

    def get_hint(self, key):
        v = C.c_double()
        check(self.backend.lib, self.backend.lib.kkamd_spgemm_get_hint(self.h, key.encode(), C.byref(v)))
        return float(v.value)

    def get_c_nnz(self): return self.get(0)
    def is_symbolic_called(self): return bool(self.get(4))
    def is_numeric_called(self): return bool(self.get(5))

    def destroy(self):
        if self.h:
            self.backend.lib.kkamd_spgemm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


_SPGEMM_ALGOS = {"SPGEMM_KK": 0, "SPGEMM_KK_DENSE": 1, "SPGEMM_KK_MEMORY": 2, "SPGEMM_KK_LP": 3, "SPGEMM_DEFAULT": 4, "SPGEMM_DEBUG": 5,
                 "SPGEMM_SERIAL": 6, "SPGEMM_KK_SPEED": 7, "SPGEMM_KK_MEMSPEED": 8}


class KokkosKernelsHandle:
    """The slice of KokkosKernels::Experimental::KokkosKernelsHandle the SpGEMM path uses
    (sparse/src/KokkosKernels_Handle.hpp:385-482): create_spgemm_handle / get_spgemm_handle /
    destroy_spgemm_handle."""

    def __init__(self, backend=None):
        self.backend = backend
        self._spgemm = None
        self._sptrsv = None
        self._spiluk = None
        self._gs = None
        self._gmres = None
        self._par_ilut = None

    def create_spgemm_handle(self, algo="SPGEMM_KK"):
        """algo: a KokkosSparse::SPGEMMAlgorithm name (sparse/src/KokkosSparse_spgemm_handle.hpp:44-93).  SPGEMM_DEBUG / SPGEMM_SERIAL
        are host-sequential in the reference and raise here (no CPU path); SPGEMM_KK_DENSE selects the dense-accumulator numeric."""
        self.backend = self.backend or torch_backend()
        if algo not in _SPGEMM_ALGOS:
            raise RuntimeError("Invalid SPGEMMAlgorithm name")
        self._spgemm = _SpgemmHandle(self.backend)
        self._spgemm.algo = algo
        self._spgemm.set("algorithm", _SPGEMM_ALGOS[algo])

    def get_spgemm_handle(self): return self._spgemm

    def destroy_spgemm_handle(self):
        if self._spgemm is not None:
            self._spgemm.destroy()
        self._spgemm = None

    def create_sptrsv_handle(self, algo, nrows, lower_tri):
        """create_sptrsv_handle(algm, nrows, lower_tri) (sparse/src/KokkosKernels_Handle.hpp:777-786); algo: a
        KokkosSparse::Experimental::SPTRSVAlgorithm name (sparse/src/KokkosSparse_sptrsv_handle.hpp:42-47)"""
        self.backend = self.backend or torch_backend()
        if algo not in _SPTRSV_ALGOS:
            raise RuntimeError("Invalid SPTRSVAlgorithm name")
        self.destroy_sptrsv_handle()
        self._sptrsv = _SptrsvHandle(self.backend, algo, nrows, lower_tri)

    def get_sptrsv_handle(self): return self._sptrsv

    def destroy_sptrsv_handle(self):
        if self._sptrsv is not None:
            self._sptrsv.destroy()
        self._sptrsv = None

    def create_spiluk_handle(self, algo, nrows, nnzL, nnzU):
        """create_spiluk_handle(algm, nrows, nnzL, nnzU) (sparse/src/KokkosKernels_Handle.hpp:853-870); algo: a
        KokkosSparse::Experimental::SPILUKAlgorithm name (sparse/src/KokkosSparse_spiluk_handle.hpp:31-33)"""
        self.backend = self.backend or torch_backend()
        if algo not in _SPILUK_ALGOS:
            raise RuntimeError("Invalid SPILUKAlgorithm name")
        self.destroy_spiluk_handle()
        self._spiluk = _SpilukHandle(self.backend, algo, nrows, nnzL, nnzU)

    def get_spiluk_handle(self): return self._spiluk

    def destroy_spiluk_handle(self):
        if self._spiluk is not None:
            self._spiluk.destroy()
        self._spiluk = None

    def create_par_ilut_handle(self, max_iter=20, residual_norm_delta_stop=1e-2, fill_in_limit=0.75, async_update=False, verbose=False):
        """create_par_ilut_handle(max_iter, residual_norm_delta_stop, fill_in_limit, async_update, verbose)
        (sparse/src/KokkosKernels_Handle.hpp:871-881)"""
        self.backend = self.backend or torch_backend()
        self.destroy_par_ilut_handle()
        self._par_ilut = _ParIlutHandle(self.backend, max_iter, residual_norm_delta_stop, fill_in_limit, async_update, verbose)

    def get_par_ilut_handle(self): return self._par_ilut

    def destroy_par_ilut_handle(self):
        if self._par_ilut is not None:
            self._par_ilut.destroy()
        self._par_ilut = None

    def create_gs_handle(self, algo="GS_DEFAULT"):
        """create_gs_handle(GSAlgorithm) (sparse/src/KokkosKernels_Handle.hpp:581-628); algo: a KokkosSparse::GSAlgorithm name
        (sparse/src/KokkosSparse_gauss_seidel_handle.hpp:30).  GS_CLUSTER and GS_TWOSTAGE raise KkamdError(UNSUPPORTED)."""
        self.backend = self.backend or torch_backend()
        if algo not in _GS_ALGOS:
            raise RuntimeError("Invalid GSAlgorithm name")
        self.destroy_gs_handle()
        self._gs = _GsHandle(self.backend, algo)

    def get_gs_handle(self): return self._gs
    def get_point_gs_handle(self): return self._gs

    def destroy_gs_handle(self):
        if self._gs is not None:
            self._gs.destroy()
        self._gs = None

    def create_gmres_handle(self, m=50, tol=1e-8, max_restart=50):
        """create_gmres_handle(m, tol, max_restart) (sparse/src/KokkosKernels_Handle.hpp); m <= 0 raises ValueError with the reference's
        text (std::invalid_argument, sparse/src/KokkosSparse_gmres_handle.hpp:116-118)"""
        self.backend = self.backend or torch_backend()
        self.destroy_gmres_handle()
        self._gmres = GMRESHandle(self.backend, m, tol, max_restart)

    def get_gmres_handle(self): return self._gmres

    def destroy_gmres_handle(self):
        if self._gmres is not None:
            self._gmres.destroy()
        self._gmres = None


_SPTRSV_ALGOS = {"SEQLVLSCHD_RP": 0, "SEQLVLSCHD_TP1": 1, "SEQLVLSCHD_TP1CHAIN": 2, "SPTRSV_CUSPARSE": 3}


class _LevelHandle:
    """What the handles of the level-scheduled routines share: the kkamd_<prefix>_create / set / get / export / destroy calls."""
    PER_LEVEL = {}   # export name -> its entries beyond num_levels; every other array has num_rows entries

    def __init__(self, backend, algo, prefix, *create_args):
        self.backend, self.algo, self.prefix = backend, algo, prefix
        self.h = C.c_void_p()
        check(backend.lib, self._fn("create")(C.byref(self.h), *create_args))

    def _fn(self, name): return getattr(self.backend.lib, "kkamd_%s_%s" % (self.prefix, name))

    def set(self, key, value):
        """"lanes_per_row", "chain_rows", "chain_levels" (kkamd_sptrsv_set, kkamd_spiluk_set)"""
        check(self.backend.lib, self._fn("set")(self.h, key.encode(), int(value)))

    def get(self, key):
        v = C.c_int64()
        check(self.backend.lib, self._fn("get")(self.h, key.encode(), C.byref(v)))
        return int(v.value)

    def export(self, what):
        """one of the handle's arrays (its class names them) as a host int32 array"""
        n = self.get("num_levels") + self.PER_LEVEL[what] if what in self.PER_LEVEL else self.get("num_rows")
        out = np.zeros(n, dtype=np.int32)
        check(self.backend.lib, self._fn("export")(self.h, what.encode(), out.ctypes.data_as(C.c_void_p), n))
        return out

    def get_algorithm(self): return self.algo
    def get_nrows(self): return self.get("num_rows")
    def get_num_levels(self): return self.get("num_levels")
    def is_symbolic_complete(self): return bool(self.get("symbolic_complete"))

    def destroy(self):
        if self.h:
            self._fn("destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _sub_handle(kh, getter, name, who):
    sub = getattr(kh, getter)() if kh is not None else None
    if sub is None:
        raise ValueError("KokkosSparse::%s: the given KernelHandle does not have an %s handle associated with it." % (who, name))
    return sub


class _SptrsvHandle(_LevelHandle):
    """KokkosSparse::Experimental::SPTRSVHandle as far as the level-scheduled solve uses it (sparse/src/KokkosSparse_sptrsv_handle.hpp):
    algorithm, size and triangle, the level sets of the symbolic phase, and this library's knobs.
    export: "level_list", "nodes_per_level" or "nodes_grouped_by_level"."""
    PER_LEVEL = {"nodes_per_level": 0}

    def __init__(self, backend, algo, nrows, lower_tri):
        super().__init__(backend, algo, "sptrsv", _SPTRSV_ALGOS[algo], int(nrows), 1 if lower_tri else 0)

    def is_lower_tri(self): return bool(self.get("lower_tri"))
    def is_upper_tri(self): return not self.is_lower_tri()


def sptrsv_symbolic(kh, row_map, entries):
    """KokkosSparse::sptrsv_symbolic(handle, rowmap, entries) (sparse/src/KokkosSparse_sptrsv.hpp:54-122): validates the triangle and
    builds the level sets on the device.  May be repeated."""
    th = _sub_handle(kh, "get_sptrsv_handle", "SPTRSV", "sptrsv_symbolic")
    be, lib = th.backend, th.backend.lib
    check(lib, lib.kkamd_sptrsv_symbolic(th.h, int(row_map.shape[0]) - 1, be.ptr(row_map), be.ptr(entries), _offset_type(row_map), be.stream()))


def sptrsv_solve(kh, row_map, entries, values, b, x):
    """KokkosSparse::sptrsv_solve(handle, rowmap, entries, values, b, x) (sparse/src/KokkosSparse_sptrsv.hpp:268-411): x := A^-1 b on the
    backend's current stream; b may be x.  b and x are rank 1 and contiguous."""
    th = _sub_handle(kh, "get_sptrsv_handle", "SPTRSV", "sptrsv_solve")
    be, lib = th.backend, th.backend.lib
    if len(b.shape) != 1 or len(x.shape) != 1:
        raise RuntimeError("KokkosSparse::sptrsv_solve: b and x must have rank 1")
    n = int(row_map.shape[0]) - 1
    if b.shape[0] != n or x.shape[0] != n:
        raise RuntimeError("KokkosSparse::sptrsv_solve: Dimensions do not match: A: %d x %d, b: %d, x: %d" % (n, n, b.shape[0], x.shape[0]))
    if _vec_stride(b, "sptrsv_solve") != 1 or _vec_stride(x, "sptrsv_solve") != 1:
        raise RuntimeError("KokkosSparse::sptrsv_solve: b and x must be contiguous")
    if _np_dtype(values) != _np_dtype(x) or _np_dtype(b) != _np_dtype(x):
        raise RuntimeError("KokkosSparse::sptrsv_solve: values, b and x must have one scalar type")
    try:
        check(lib, lib.kkamd_sptrsv_solve(th.h, n, be.ptr(row_map), be.ptr(entries), be.ptr(values), be.ptr(b), be.ptr(x),
                                          _offset_type(row_map), _scalar_type(x), be.stream()))
    except _capi.KkamdError as e:
        if e.status == _capi.ERR_STATE:
            raise ValueError(str(e))   # std::invalid_argument in the reference
        raise
    return x


_SPILUK_ALGOS = {"SEQLVLSCHD_TP1": 0}


class _SpilukHandle(_LevelHandle):
    """KokkosSparse::Experimental::SPILUKHandle as far as the level-scheduled factorisation uses it
    (sparse/src/KokkosSparse_spiluk_handle.hpp): algorithm, size, nnzL and nnzU, the level sets of L, and this library's knobs.
    export: "level_list" (1-based), "level_ptr" (num_levels + 1) or "level_idx"."""
    PER_LEVEL = {"level_ptr": 1}

    def __init__(self, backend, algo, nrows, nnzL, nnzU):
        super().__init__(backend, algo, "spiluk", _SPILUK_ALGOS[algo], int(nrows), int(nnzL), int(nnzU))

    def get_nnzL(self): return self.get("nnzL")
    def get_nnzU(self): return self.get("nnzU")


def spiluk_symbolic(kh, fill_lev, A_row_map, A_entries, L_row_map, L_entries, U_row_map, U_entries):
    """KokkosSparse::spiluk_symbolic(handle, fill_lev, A_rowmap, A_entries, L_rowmap, L_entries, U_rowmap, U_entries)
    (sparse/src/KokkosSparse_spiluk.hpp:42-197): writes the graphs of L and U for level of fill fill_lev and records nnzL, nnzU and the
    level sets of L in the handle.  The extents of L_entries / U_entries are the capacities.  May be repeated."""
    ih = _sub_handle(kh, "get_spiluk_handle", "SPILUK", "spiluk_symbolic")
    be, lib = ih.backend, ih.backend.lib
    n = int(A_row_map.shape[0]) - 1
    if L_row_map.shape[0] != n + 1 or U_row_map.shape[0] != n + 1:
        raise RuntimeError("KokkosSparse::spiluk_symbolic: L_rowmap and U_rowmap must have A_rowmap's extent %d" % (n + 1))
    if _np_dtype(L_row_map) != _np_dtype(A_row_map) or _np_dtype(U_row_map) != _np_dtype(A_row_map):
        raise RuntimeError("KokkosSparse::spiluk_symbolic: A_rowmap, L_rowmap and U_rowmap must have one offset type")
    check(lib, lib.kkamd_spiluk_symbolic(ih.h, int(fill_lev), n, be.ptr(A_row_map), be.ptr(A_entries), be.ptr(L_row_map), be.ptr(L_entries),
                                         int(L_entries.shape[0]), be.ptr(U_row_map), be.ptr(U_entries), int(U_entries.shape[0]),
                                         _offset_type(A_row_map), be.stream()))


def spiluk_numeric(kh, fill_lev, A_row_map, A_entries, A_values, L_row_map, L_entries, L_values, U_row_map, U_entries, U_values):
    """KokkosSparse::spiluk_numeric(handle, fill_lev, A_rowmap, A_entries, A_values, L_rowmap, L_entries, L_values, U_rowmap, U_entries,
    U_values) (sparse/src/KokkosSparse_spiluk.hpp:200-415): the ILU(k) factors of A on the analysed pattern, on the backend's current
    stream.  New values of A need no second symbolic call."""
    ih = _sub_handle(kh, "get_spiluk_handle", "SPILUK", "spiluk_numeric")
    be, lib = ih.backend, ih.backend.lib
    n = int(A_row_map.shape[0]) - 1
    if _np_dtype(L_values) != _np_dtype(A_values) or _np_dtype(U_values) != _np_dtype(A_values):
        raise RuntimeError("KokkosSparse::spiluk_numeric: A_values, L_values and U_values must have one scalar type")
    if _np_dtype(L_row_map) != _np_dtype(A_row_map) or _np_dtype(U_row_map) != _np_dtype(A_row_map):
        raise RuntimeError("KokkosSparse::spiluk_numeric: A_rowmap, L_rowmap and U_rowmap must have one offset type")
    if ih.is_symbolic_complete() and (L_values.shape[0] < ih.get_nnzL() or U_values.shape[0] < ih.get_nnzU()):
        raise RuntimeError("KokkosSparse::spiluk_numeric: L_values / U_values are shorter than nnzL / nnzU")
    try:
        check(lib, lib.kkamd_spiluk_numeric(ih.h, int(fill_lev), n, be.ptr(A_row_map), be.ptr(A_entries), be.ptr(A_values), be.ptr(L_row_map),
                                            be.ptr(L_entries), be.ptr(L_values), be.ptr(U_row_map), be.ptr(U_entries), be.ptr(U_values),
                                            _offset_type(A_row_map), _scalar_type(A_values), be.stream()))
    except _capi.KkamdError as e:
        if e.status == _capi.ERR_STATE:
            raise ValueError(str(e))   # std::invalid_argument in the reference
        raise


class _ParIlutHandle:
    """KokkosSparse::Experimental::PAR_ILUTHandle (sparse/src/KokkosSparse_par_ilut_handle.hpp:55-200): the five inputs, nnzL / nnzU /
    nrows of the symbolic phase, the statistics of the numeric phase, and this library's knob "lanes_per_row"."""

    def __init__(self, backend, max_iter, residual_norm_delta_stop, fill_in_limit, async_update, verbose):
        self.backend = backend
        self.h = C.c_void_p()
        check(backend.lib, backend.lib.kkamd_par_ilut_create(C.byref(self.h), int(max_iter), float(residual_norm_delta_stop), float(fill_in_limit),
                                                             1 if async_update else 0, 1 if verbose else 0))

    def set(self, key, value): check(self.backend.lib, self.backend.lib.kkamd_par_ilut_set(self.h, key.encode(), float(value)))

    def get(self, key):
        v = C.c_int64()
        check(self.backend.lib, self.backend.lib.kkamd_par_ilut_get(self.h, key.encode(), C.byref(v)))
        return int(v.value)

    def get_real(self, key):
        v = C.c_double()
        check(self.backend.lib, self.backend.lib.kkamd_par_ilut_get_real(self.h, key.encode(), C.byref(v)))
        return float(v.value)

    def get_nrows(self): return self.get("num_rows")
    def get_nnzL(self): return self.get("nnzL")
    def get_nnzU(self): return self.get("nnzU")
    def get_max_iter(self): return self.get("max_iter")
    def set_max_iter(self, v): self.set("max_iter", v)
    def get_residual_norm_delta_stop(self): return self.get_real("residual_norm_delta_stop")
    def set_residual_norm_delta_stop(self, v): self.set("residual_norm_delta_stop", v)
    def get_fill_in_limit(self): return self.get_real("fill_in_limit")
    def set_fill_in_limit(self, v): self.set("fill_in_limit", v)
    def get_async_update(self): return bool(self.get("async_update"))
    def set_async_update(self, v): self.set("async_update", 1 if v else 0)
    def get_verbose(self): return bool(self.get("verbose"))
    def set_verbose(self, v): self.set("verbose", 1 if v else 0)
    def get_num_iters(self): return self.get("num_iters")
    def get_end_rel_res(self): return self.get_real("end_rel_res")
    def is_symbolic_complete(self): return bool(self.get("symbolic_complete"))

    def destroy(self):
        if self.h:
            self.backend.lib.kkamd_par_ilut_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def par_ilut_symbolic(kh, A_row_map, A_entries, L_row_map, U_row_map):
    """KokkosSparse::Experimental::par_ilut_symbolic(handle, A_rowmap, A_entries, L_rowmap, U_rowmap) (sparse/src/KokkosSparse_par_ilut.hpp:76-190):
    writes the row maps of the initial L and U and records nnzL, nnzU and the size in the handle."""
    ih = _sub_handle(kh, "get_par_ilut_handle", "PAR_ILUT", "par_ilut_symbolic")
    be, lib = ih.backend, ih.backend.lib
    n = int(A_row_map.shape[0]) - 1
    if L_row_map.shape[0] != n + 1 or U_row_map.shape[0] != n + 1:
        raise RuntimeError("KokkosSparse::par_ilut_symbolic: L_rowmap and U_rowmap must have A_rowmap's extent %d" % (n + 1))
    if _np_dtype(L_row_map) != _np_dtype(A_row_map) or _np_dtype(U_row_map) != _np_dtype(A_row_map):
        raise RuntimeError("KokkosSparse::par_ilut_symbolic: A_rowmap, L_rowmap and U_rowmap must have one offset type")
    check(lib, lib.kkamd_par_ilut_symbolic(ih.h, n, be.ptr(A_row_map), be.ptr(A_entries), be.ptr(L_row_map), be.ptr(U_row_map),
                                           _offset_type(A_row_map), be.stream()))


def par_ilut_numeric(kh, A_row_map, A_entries, A_values, L_row_map, U_row_map):
    """KokkosSparse::Experimental::par_ilut_numeric (sparse/src/KokkosSparse_par_ilut.hpp:207-380).  The reference resizes the caller's
    views; here the final row maps are written into L_row_map / U_row_map and the factors are returned as new arrays:
    (L_entries, L_values, U_entries, U_values).  May be repeated with new values."""
    ih = _sub_handle(kh, "get_par_ilut_handle", "PAR_ILUT", "par_ilut_numeric")
    be, lib = ih.backend, ih.backend.lib
    n = int(A_row_map.shape[0]) - 1
    if _np_dtype(L_row_map) != _np_dtype(A_row_map) or _np_dtype(U_row_map) != _np_dtype(A_row_map):
        raise RuntimeError("KokkosSparse::par_ilut_numeric: A_rowmap, L_rowmap and U_rowmap must have one offset type")
    try:
        check(lib, lib.kkamd_par_ilut_numeric(ih.h, n, be.ptr(A_row_map), be.ptr(A_entries), be.ptr(A_values), be.ptr(L_row_map), be.ptr(U_row_map),
                                              _offset_type(A_row_map), _scalar_type(A_values), be.stream()))
    except _capi.KkamdError as e:
        if e.status == _capi.ERR_STATE:
            raise ValueError(str(e))   # std::invalid_argument in the reference
        raise
    nl, nu = ih.get("nnzL_out"), ih.get("nnzU_out")
    vdt = _np_dtype(A_values)
    L_ent, L_val, U_ent, U_val = be.empty(nl, np.int32), be.empty(nl, vdt), be.empty(nu, np.int32), be.empty(nu, vdt)
    check(lib, lib.kkamd_par_ilut_copy_factors(ih.h, be.ptr(L_ent), be.ptr(L_val), nl, be.ptr(U_ent), be.ptr(U_val), nu, be.stream()))
    return L_ent, L_val, U_ent, U_val


_GS_ALGOS = {"GS_DEFAULT": 0, "GS_PERMUTED": 1, "GS_TEAM": 2, "GS_CLUSTER": 3, "GS_TWOSTAGE": 4}


class _GsHandle(_LevelHandle):
    """KokkosSparse::PointGaussSeidelHandle as far as the multicolor sweep uses it (sparse/src/KokkosSparse_gauss_seidel_handle.hpp):
    algorithm, the colouring, the permutation, the long-row threshold, and this library's knobs (a colour is a level of the schedule).
    export: "colors" (1-based), "color_xadj" (num_colors + 1), "color_adj" (the rows grouped by colour) or "old_to_new"."""
    PER_LEVEL = {"color_xadj": 1}

    def __init__(self, backend, algo):
        super().__init__(backend, algo, "gs", _GS_ALGOS[algo])

    def get_algorithm_type(self): return self.algo
    def get_num_colors(self): return self.get("num_colors")
    def is_numeric_called(self): return bool(self.get("numeric_complete"))
    def set_long_row_threshold(self, lrt): self.set("long_row_threshold", lrt)
    def get_long_row_threshold(self): return self.get("long_row_threshold")


def gauss_seidel_symbolic(kh, num_rows, num_cols, row_map, entries, is_graph_symmetric=True, colors=None):
    """KokkosSparse::gauss_seidel_symbolic(handle, num_rows, num_cols, row_map, entries, is_graph_symmetric)
    (sparse/src/KokkosSparse_gauss_seidel.hpp:45-134): colours the graph on the device (of A + A^T unless is_graph_symmetric), groups
    and permutes.  colors: None, or an int32 array of the caller's 1-based colours, validated.  May be repeated."""
    gh = _sub_handle(kh, "get_gs_handle", "GS", "gauss_seidel_symbolic")
    be, lib = gh.backend, gh.backend.lib
    if int(row_map.shape[0]) != int(num_rows) + 1:
        raise RuntimeError("KokkosSparse::gauss_seidel_symbolic: row_map has %d entries, not num_rows + 1 = %d" % (row_map.shape[0], num_rows + 1))
    if colors is not None and (colors.shape[0] != num_rows or _np_dtype(colors) != np.dtype(np.int32)):
        raise RuntimeError("KokkosSparse::gauss_seidel_symbolic: colors must hold num_rows int32 entries")
    check(lib, lib.kkamd_gs_symbolic(gh.h, int(num_rows), int(num_cols), be.ptr(row_map), be.ptr(entries), _offset_type(row_map),
                                     1 if is_graph_symmetric else 0, be.ptr(colors), be.stream()))


def gauss_seidel_numeric(kh, num_rows, num_cols, row_map, entries, values, given_inverse_diagonal=None, is_graph_symmetric=True):
    """KokkosSparse::gauss_seidel_numeric(handle, num_rows, num_cols, row_map, entries, values[, given_inverse_diagonal],
    is_graph_symmetric) (sparse/src/KokkosSparse_gauss_seidel.hpp:173-370); a bool in the place of given_inverse_diagonal is the
    reference's shorter overload.  New values need no second symbolic call."""
    gh = _sub_handle(kh, "get_gs_handle", "GS", "gauss_seidel_numeric")
    be, lib = gh.backend, gh.backend.lib
    if isinstance(given_inverse_diagonal, bool):
        given_inverse_diagonal = None
    if given_inverse_diagonal is not None and (given_inverse_diagonal.shape[0] != num_rows or _np_dtype(given_inverse_diagonal) != _np_dtype(values)
                                               or _vec_stride(given_inverse_diagonal, "gauss_seidel_numeric") != 1):
        raise RuntimeError("KokkosSparse::gauss_seidel_numeric: given_inverse_diagonal must hold num_rows contiguous entries of the values' type")
    try:
        check(lib, lib.kkamd_gs_numeric(gh.h, int(num_rows), int(num_cols), be.ptr(row_map), be.ptr(entries), be.ptr(values),
                                        be.ptr(given_inverse_diagonal), _offset_type(row_map), _scalar_type(values), be.stream()))
    except _capi.KkamdError as e:
        if e.status == _capi.ERR_STATE:
            raise ValueError(str(e))
        raise


def _gs_apply(who, direction, kh, num_rows, num_cols, row_map, entries, values, x, y, init_zero_x_vector, update_y_vector, omega, num_iter):
    gh = _sub_handle(kh, "get_gs_handle", "GS", who)
    be, lib = gh.backend, gh.backend.lib
    if y is None and not update_y_vector:
        y = x[:num_rows]                                    # never read: the handle's permuted y of the previous apply is used
    if len(x.shape) != len(y.shape) or len(x.shape) not in (1, 2):
        raise RuntimeError("KokkosSparse::%s: x and y must both have rank 1 or both rank 2" % who)
    nv = int(x.shape[1]) if len(x.shape) == 2 else 1
    if x.shape[0] < num_cols or y.shape[0] < num_rows or (len(y.shape) == 2 and y.shape[1] != nv) or nv < 1:
        raise RuntimeError("KokkosSparse::%s: Dimensions do not match: A: %d x %d, x: %s, y: %s" % (who, num_rows, num_cols, tuple(x.shape), tuple(y.shape)))
    if _np_dtype(x) != _np_dtype(values) or _np_dtype(y) != _np_dtype(values):
        raise RuntimeError("KokkosSparse::%s: values, x and y must have one scalar type" % who)
    if len(x.shape) == 1:
        xs, ys = (_vec_stride(x, who), 0), (_vec_stride(y, who), 0)
    else:
        xs, ys = _strides(x), _strides(y)
        if min(xs) < 0 or min(ys) < 0:
            raise RuntimeError("KokkosSparse::%s: negative strides are not supported" % who)
    try:
        check(lib, lib.kkamd_gs_apply(gh.h, int(num_rows), int(num_cols), be.ptr(row_map), be.ptr(entries), be.ptr(values), be.ptr(x), xs[0], xs[1],
                                      be.ptr(y), ys[0], ys[1], nv, 1 if init_zero_x_vector else 0, 1 if update_y_vector else 0, float(omega),
                                      int(num_iter), direction, _offset_type(row_map), _scalar_type(values), be.stream()))
    except _capi.KkamdError as e:
        if e.status == _capi.ERR_STATE:
            raise ValueError(str(e))
        raise
    return x


def symmetric_gauss_seidel_apply(kh, num_rows, num_cols, row_map, entries, values, x_lhs_output_vec, y_rhs_input_vec, init_zero_x_vector=False,
                                 update_y_vector=True, omega=1.0, numIter=1):
    """KokkosSparse::symmetric_gauss_seidel_apply (sparse/src/KokkosSparse_gauss_seidel.hpp:372-500): numIter times a forward and then a
    backward sweep, on the backend's current stream.  x: num_cols rows, y: num_rows rows, rank 1 or rank 2 in any layout."""
    return _gs_apply("symmetric_gauss_seidel_apply", _capi.GS_SYMMETRIC, kh, num_rows, num_cols, row_map, entries, values, x_lhs_output_vec,
                     y_rhs_input_vec, init_zero_x_vector, update_y_vector, omega, numIter)


def forward_sweep_gauss_seidel_apply(kh, num_rows, num_cols, row_map, entries, values, x_lhs_output_vec, y_rhs_input_vec, init_zero_x_vector=False,
                                     update_y_vector=True, omega=1.0, numIter=1):
    """KokkosSparse::forward_sweep_gauss_seidel_apply (sparse/src/KokkosSparse_gauss_seidel.hpp:502-630): colours 1..C, numIter times"""
    return _gs_apply("forward_sweep_gauss_seidel_apply", _capi.GS_FORWARD, kh, num_rows, num_cols, row_map, entries, values, x_lhs_output_vec,
                     y_rhs_input_vec, init_zero_x_vector, update_y_vector, omega, numIter)


def backward_sweep_gauss_seidel_apply(kh, num_rows, num_cols, row_map, entries, values, x_lhs_output_vec, y_rhs_input_vec, init_zero_x_vector=False,
                                      update_y_vector=True, omega=1.0, numIter=1):
    """KokkosSparse::backward_sweep_gauss_seidel_apply (sparse/src/KokkosSparse_gauss_seidel.hpp:632-760): colours C..1, numIter times"""
    return _gs_apply("backward_sweep_gauss_seidel_apply", _capi.GS_BACKWARD, kh, num_rows, num_cols, row_map, entries, values, x_lhs_output_vec,
                     y_rhs_input_vec, init_zero_x_vector, update_y_vector, omega, numIter)


class GMRESHandle:
    """KokkosSparse::Experimental::GMRESHandle (sparse/src/KokkosSparse_gmres_handle.hpp:38-181): m, tol, max_restart, ortho, verbose, the
    results of the last solve, and this library's knobs ("fuse", "rows_per_group": kkamd_gmres_set) and workspace."""
    ORTHO = {"CGS2": 0, "MGS": 1}
    FLAGS = ("Conv", "NoConv", "LOA", "NotRun")

    def __init__(self, backend, m=50, tol=1e-8, max_restart=50):
        self.backend = backend
        self.h = C.c_void_p()
        try:
            check(backend.lib, backend.lib.kkamd_gmres_create(C.byref(self.h), int(m), float(tol), int(max_restart)))
        except _capi.KkamdError as e:
            if e.status == _capi.ERR_INVALID_ARG:
                raise ValueError(str(e))
            raise

    def set(self, key, value):
        check(self.backend.lib, self.backend.lib.kkamd_gmres_set(self.h, key.encode(), int(value)))

    def get(self, key):
        v = C.c_int64()
        check(self.backend.lib, self.backend.lib.kkamd_gmres_get(self.h, key.encode(), C.byref(v)))
        return int(v.value)

    def get_real(self, key):
        v = C.c_double()
        check(self.backend.lib, self.backend.lib.kkamd_gmres_get_real(self.h, key.encode(), C.byref(v)))
        return float(v.value)

    def export(self, what):
        """"short_residuals", "true_residuals", "hessenberg" ((m + 1) x m) or "basis" (n x (m + 1)) of the last solve, as float64"""
        m = self.get("m")
        if what == "hessenberg":
            shape = (m + 1, m) if self.get("num_short_residuals") or self.get("num_true_residuals") else (0, 0)
        elif what == "basis":
            shape = (self.get("num_rows"), m + 1)
        elif what in ("precond_ms", "spmv_ms", "ortho_ms"):
            shape = (self.get("num_short_residuals") if self.get("profile") else 0,)
        else:
            shape = (self.get("num_" + what),)
        out = np.zeros(int(np.prod(shape)), dtype=np.float64)
        check(self.backend.lib, self.backend.lib.kkamd_gmres_export(self.h, what.encode(), out.ctypes.data_as(C.c_void_p), out.size))
        return out.reshape(shape, order="F")

    def get_m(self): return self.get("m")
    def set_m(self, m): self.set("m", m)
    def get_max_restart(self): return self.get("max_restart")
    def set_max_restart(self, r): self.set("max_restart", r)
    def get_tol(self): return self.get_real("tol")
    def set_tol(self, tol): check(self.backend.lib, self.backend.lib.kkamd_gmres_set_tol(self.h, float(tol)))
    def get_ortho(self): return ("CGS2", "MGS")[self.get("ortho")]

    def set_ortho(self, ortho):
        if ortho not in self.ORTHO:
            raise ValueError("Invalid argument for 'ortho'.  Please use 'CGS2' or 'MGS'.")
        self.set("ortho", self.ORTHO[ortho])

    def get_verbose(self): return bool(self.get("verbose"))
    def set_verbose(self, v): self.set("verbose", 1 if v else 0)

    def reset_handle(self, m=50, tol=1e-8, max_restart=50):
        check(self.backend.lib, self.backend.lib.kkamd_gmres_reset(self.h, int(m), float(tol), int(max_restart)))

    def get_conv_flag_val(self): return self.FLAGS[self.get("conv_flag")]

    def get_num_iters(self):
        """the reference asserts that a solve has run (gmres_handle.hpp:165-168)"""
        if self.get_conv_flag_val() == "NotRun":
            raise AssertionError("get_num_iters: GMRES was never run")
        return self.get("num_iters")

    def get_end_rel_res(self):
        if self.get_conv_flag_val() == "NotRun":
            raise AssertionError("get_end_rel_res: GMRES was never run")
        return self.get_real("end_rel_res")

    def destroy(self):
        if self.h:
            self.backend.lib.kkamd_gmres_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Preconditioner:
    """KokkosSparse::Experimental::Preconditioner (sparse/src/KokkosSparse_Preconditioner.hpp:55-112) over a kkamd_precond_t.  A subclass
    that overrides apply_device(d_x, d_y, alpha, beta, value_type, stream) -- raw device pointers -- and calls _init_callback() is a
    foreign preconditioner (kkamd_precond_create_callback)."""

    def __init__(self, backend=None):
        self.backend = backend or torch_backend()
        self.p = C.c_void_p()
        self._keep = ()

    def _init_callback(self):
        def tramp(ctx, d_x, d_y, alpha, beta, value_type, stream):
            try:
                return int(self.apply_device(d_x, d_y, alpha, beta, value_type, stream) or 0)
            except _capi.KkamdError as e:
                return e.status
        self._fn = _capi.PRECOND_FN(tramp)
        check(self.backend.lib, self.backend.lib.kkamd_precond_create_callback(C.byref(self.p), self._fn, None))

    def apply(self, X, Y, transM="N", alpha=1.0, beta=0.0):
        """Y := alpha * M X + beta * Y on the backend's current stream"""
        if transM[0] not in "Nn":
            raise RuntimeError("Preconditioner::apply only supports 'N' for transM")
        if _np_dtype(X) != _np_dtype(Y) or X.shape[0] != Y.shape[0] or _vec_stride(X, "apply") != 1 or _vec_stride(Y, "apply") != 1:
            raise RuntimeError("Preconditioner::apply: X and Y must be contiguous rank-1 arrays of one length and scalar type")
        be = self.backend
        check(be.lib, be.lib.kkamd_precond_apply(self.p, be.ptr(X), be.ptr(Y), float(alpha), float(beta), _scalar_type(X), be.stream()))
        return Y

    def isInitialized(self): return True
    def isComputed(self): return True
    def hasTransposeApply(self): return False

    def destroy(self):
        if self.p:
            self.backend.lib.kkamd_precond_destroy(self.p)
            self.p = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class MatrixPrec(Preconditioner):
    """KokkosSparse::Experimental::MatrixPrec (sparse/src/KokkosSparse_MatrixPrec.hpp:45-101): apply is an SpMV with the given matrix"""

    def __init__(self, mat):
        super().__init__(mat.backend)
        self._keep = (mat,)
        d = mat.desc()
        check(self.backend.lib, self.backend.lib.kkamd_precond_create_matrix(C.byref(self.p), C.byref(d), self.backend.stream()))


class LUPrec(Preconditioner):
    """KokkosSparse::Experimental::LUPrec (sparse/src/KokkosSparse_LUPrec.hpp:43-119): Y := alpha * U^-1 L^-1 X + beta * Y.  The two
    triangular solves are analysed once, here (the reference analyses at every apply, :94-98)."""

    def __init__(self, L, U):
        super().__init__(L.backend)
        if L.numRows() != U.numRows():
            raise RuntimeError("LUPrec: L.numRows() != U.numRows()")
        self._keep = (L, U)
        dl, du = L.desc(), U.desc()
        check(self.backend.lib, self.backend.lib.kkamd_precond_create_lu(C.byref(self.p), C.byref(dl), C.byref(du), self.backend.stream()))


def gmres(kh, A, B, X, precond=None):
    """KokkosSparse::Experimental::gmres(handle, A, B, X, precond) (sparse/src/KokkosSparse_gmres.hpp:58-158): solves A X = B from the
    initial guess in X with restarted GMRES, right-preconditioned when precond is given; results in the handle
    (get_num_iters / get_end_rel_res / get_conv_flag_val).  Breakdown and a NaN residual raise RuntimeError with the reference's text."""
    gh = _sub_handle(kh, "get_gmres_handle", "GMRES", "gmres")
    be, lib = gh.backend, gh.backend.lib
    if len(B.shape) != 1 or len(X.shape) != 1:
        raise RuntimeError("gmres: B and X must have rank 1")
    if X.shape[0] != B.shape[0] or A.numCols() != X.shape[0] or A.numRows() != B.shape[0]:
        raise RuntimeError("KokkosSparse::gmres: Dimensions do not match: , A: %d x %d, x: %d, b: %d" % (A.numRows(), A.numCols(), X.shape[0], B.shape[0]))
    if _vec_stride(B, "gmres") != 1 or _vec_stride(X, "gmres") != 1:
        raise RuntimeError("KokkosSparse::gmres: B and X must be contiguous")
    if _np_dtype(B) != _np_dtype(X):
        raise RuntimeError("gmres: B and X must have one scalar type")
    d = A.desc()
    try:
        check(lib, lib.kkamd_gmres_solve(gh.h, C.byref(d), be.ptr(B), be.ptr(X), precond.p if precond is not None else None, _scalar_type(X),
                                         be.stream()))
    except _capi.KkamdError as e:
        if e.status in (_capi.ERR_INVALID_ARG, _capi.ERR_NUMERIC):
            raise RuntimeError(str(e))
        raise
    return X


def spgemm_symbolic(kh, A, transposeA, B, transposeB, Cmat=None, allocate=True):
    """Matrix-level KokkosSparse::spgemm_symbolic (sparse/src/KokkosSparse_spgemm.hpp:40-61): allocates
    row_map C, runs the symbolic phase, allocates entries/values of get_c_nnz() and returns C.
    allocate=False (view-level behaviour, :spgemm_symbolic with row maps only) returns the row_map of C alone."""
    if transposeA or transposeB:
        raise RuntimeError("KokkosSparse::spgemm_symbolic: transposing A or B is not yet supported")
    sh = kh.get_spgemm_handle() if kh is not None else None
    if sh is None:
        raise ValueError("KokkosSparse::spgemm_symbolic: the given KernelHandle does not have an SpGEMM handle "
                         "associated with it.")
    if A.numCols() != B.numRows():
        raise RuntimeError("KokkosSparse::spgemm: A.numCols() != B.numRows()")
    be, lib = A.backend, A.backend.lib
    m, n, k = A.numRows(), A.numCols(), B.numCols()
    odt = _np_dtype(A.graph.row_map)
    rmC = be.empty(m + 1, odt)
    nnz = C.c_int64()
    check(lib, lib.kkamd_spgemm_symbolic(sh.h, m, n, k, be.ptr(A.graph.row_map), be.ptr(A.graph.entries),
                                         be.ptr(B.graph.row_map), be.ptr(B.graph.entries), be.ptr(rmC),
                                         _offset_type(A.graph.row_map), C.byref(nnz), be.stream()))
    if not allocate:
        return rmC
    vdt = _np_dtype(A.values) if A.values is not None else np.dtype(np.float64)
    return CrsMatrix(m, k, rmC, be.empty(nnz.value, np.int32), be.empty(nnz.value, vdt), backend=be)


def spgemm_numeric(kh, A, transposeA, B, transposeB, Cmat):
    if transposeA or transposeB:
        raise RuntimeError("KokkosSparse::spgemm_numeric: transposing A or B is not yet supported")
    sh = kh.get_spgemm_handle() if kh is not None else None
    if sh is None:
        raise ValueError("KokkosSparse::spgemm_numeric: the given KernelHandle does not have an SpGEMM handle "
                         "associated with it.")
    be, lib = A.backend, A.backend.lib
    # the library keeps entries(C) across numeric calls into the SAME arrays; whether these are the same it can only judge by address,
    # and a caching allocator hands a freed address out again: arrays this wrapper has not yet seen through THIS handle are told to be
    # new ("entries_computed" 0), whatever their address
    seen = (id(sh), id(Cmat.graph.entries), be.ptr(Cmat.graph.entries))
    if getattr(Cmat, "_kk_numeric_seen", None) != seen:
        sh.set("entries_computed", 0)
    try:
        check(lib, lib.kkamd_spgemm_numeric(sh.h, A.numRows(), A.numCols(), B.numCols(), be.ptr(A.graph.row_map),
                                            be.ptr(A.graph.entries), be.ptr(A.values), be.ptr(B.graph.row_map),
                                            be.ptr(B.graph.entries), be.ptr(B.values), be.ptr(Cmat.graph.row_map),
                                            be.ptr(Cmat.graph.entries), be.ptr(Cmat.values),
                                            _offset_type(A.graph.row_map), _scalar_type(A.values), be.stream()))
    except _capi.KkamdError as e:
        if e.status == _capi.ERR_STATE:
            raise ValueError(str(e))   # std::invalid_argument in the reference
        raise
    Cmat._kk_numeric_seen = seen
    return Cmat


def spgemm_jacobi(kh, A, transposeA, B, transposeB, Cmat, omega, dinv):
    """KokkosSparse::Experimental::spgemm_jacobi (sparse/src/KokkosSparse_spgemm_jacobi.hpp:26-188) on matrices: C = B - omega D^-1 (A B) into
    the C that spgemm_symbolic(kh, A, False, B, False) returned, in the place of spgemm_numeric.  dinv: A.numRows() values of A's value
    type, rank 1 or rank 2 with one column."""
    if transposeA or transposeB:
        raise RuntimeError("spgemm-jacobi does not support transposed multiply. If you need this case please let kokkos-kernels developers know.\n")
    sh = kh.get_spgemm_handle() if kh is not None else None
    if sh is None:
        raise ValueError("KokkosSparse::spgemm_jacobi: the given KernelHandle does not have an SpGEMM handle associated with it.")
    be, lib = A.backend, A.backend.lib
    if dinv is not None:
        shape = tuple(int(v) for v in dinv.shape)
        if shape not in ((A.numRows(),), (A.numRows(), 1)) or _np_dtype(dinv) != _np_dtype(A.values):
            raise RuntimeError("KokkosSparse::spgemm_jacobi: dinv must hold A.numRows() values of A's value type (rank 1, or rank 2 with one column)")
    seen = (id(sh), id(Cmat.graph.entries), be.ptr(Cmat.graph.entries))      # see spgemm_numeric: arrays not yet seen through this handle are new
    if getattr(Cmat, "_kk_numeric_seen", None) != seen:
        sh.set("entries_computed", 0)
    try:
        check(lib, lib.kkamd_spgemm_jacobi(sh.h, A.numRows(), A.numCols(), B.numCols(), be.ptr(A.graph.row_map), be.ptr(A.graph.entries), be.ptr(A.values),
                                           be.ptr(B.graph.row_map), be.ptr(B.graph.entries), be.ptr(B.values), be.ptr(Cmat.graph.row_map),
                                           be.ptr(Cmat.graph.entries), be.ptr(Cmat.values), float(omega), be.ptr(dinv),
                                           _offset_type(A.graph.row_map), _scalar_type(A.values), be.stream()))
    except _capi.KkamdError as e:
        if e.status == _capi.ERR_STATE:
            raise ValueError(str(e))   # std::invalid_argument in the reference
        raise
    Cmat._kk_numeric_seen = seen
    return Cmat


def spgemm(A, transposeA, B, transposeB):
    """No-reuse KokkosSparse::spgemm<CMatrix>(A, false, B, false) (sparse/src/KokkosSparse_spgemm.hpp:170-218)."""
    kh = KokkosKernelsHandle(A.backend)
    kh.create_spgemm_handle()
    try:
        Cm = spgemm_symbolic(kh, A, transposeA, B, transposeB)
        spgemm_numeric(kh, A, transposeA, B, transposeB, Cm)
    finally:
        kh.destroy_spgemm_handle()
    return Cm


_MIS2_ALGOS = {"MIS2_QUALITY": _capi.MIS2_QUALITY, "MIS2_FAST": _capi.MIS2_FAST}
MIS2_STATS = ("rounds", "masked_rounds", "host_syncs", "launches", "primary_aggregates", "secondary_aggregates", "unlabelled_before_phase3",
              "scratch_bytes")


def mis2_algorithm_name(algo):
    """KokkosGraph::mis2_algorithm_name (graph/src/KokkosGraph_MIS2.hpp:81-87)"""
    return algo if algo in _MIS2_ALGOS else "*** Invalid MIS2 algo enum value.\n"


def _mis2_graph(who, row_map, entries, backend):
    be = backend or torch_backend()
    if not hasattr(be.lib, "kkamd_graph_d2_mis"):
        raise RuntimeError("KokkosGraph::%s: the loaded library does not export the MIS-2 unit" % who)
    n = max(int(row_map.shape[0]) - 1, 0)
    if _np_dtype(entries) != np.dtype(np.int32):
        raise RuntimeError("KokkosGraph::%s: entries must be int32" % who)
    return be, be.lib, n


def graph_d2_mis(row_map, entries, algo="MIS2_FAST", backend=None, stats=None):
    """KokkosGraph::graph_d2_mis<device>(rowmap, colinds, algo) (graph/src/KokkosGraph_MIS2.hpp:31-49): the vertices of a distance-2
    maximal independent set of a symmetric graph, ascending.  stats: None, or a dict that receives the MIS2_STATS."""
    be, lib, n = _mis2_graph("graph_d2_mis", row_map, entries, backend)
    if algo not in _MIS2_ALGOS:
        raise ValueError("graph_d2_mis: invalid algorithm")
    mis = be.empty(max(n, 1), np.int32)
    cnt = C.c_int64()
    st = (C.c_int64 * 8)()
    check(lib, lib.kkamd_graph_d2_mis(n, be.ptr(row_map), _offset_type(row_map), be.ptr(entries), _MIS2_ALGOS[algo], be.ptr(mis), C.byref(cnt), st,
                                      be.stream()))
    if stats is not None:
        stats.update(zip(MIS2_STATS, list(st)))
    return mis[:cnt.value]


def _mis2_labels(who, secondary, row_map, entries, backend, stats):
    be, lib, n = _mis2_graph(who, row_map, entries, backend)
    labels = be.empty(max(n, 1), np.int32)
    cnt = C.c_int64()
    st = (C.c_int64 * 8)()
    check(lib, lib.kkamd_graph_mis2_aggregate(n, be.ptr(row_map), _offset_type(row_map), be.ptr(entries), secondary, be.ptr(labels), C.byref(cnt), st,
                                              be.stream()))
    if stats is not None:
        stats.update(zip(MIS2_STATS, list(st)))
    return labels[:n], cnt.value


def graph_mis2_coarsen(row_map, entries, backend=None, stats=None):
    """KokkosGraph::graph_mis2_coarsen<device>(rowmap, colinds, numClusters) (graph/src/KokkosGraph_MIS2.hpp:51-64): (labels, numClusters)"""
    return _mis2_labels("graph_mis2_coarsen", 0, row_map, entries, backend, stats)


def graph_mis2_aggregate(row_map, entries, backend=None, stats=None):
    """KokkosGraph::graph_mis2_aggregate<device>(rowmap, colinds, numAggregates) (graph/src/KokkosGraph_MIS2.hpp:66-79): (labels,
    numAggregates), with the secondary aggregates of phase 2"""
    return _mis2_labels("graph_mis2_aggregate", 1, row_map, entries, backend, stats)


def graph_explicit_coarsen(row_map, entries, labels, num_coarse, compress=True, inverse_map=False, backend=None):
    """KokkosGraph::Experimental::graph_explicit_coarsen / graph_explicit_coarsen_with_inverse_map
    (graph/src/KokkosGraph_ExplicitCoarsening.hpp:35-92): (coarse_row_map, coarse_entries), with inverse_map also (inverse_offsets,
    inverse_labels).  One call of the C entry point, with room for nnz entries: the documented upper bound of the coarse graph."""
    be, lib, n = _mis2_graph("graph_explicit_coarsen", row_map, entries, backend)
    nc = int(num_coarse)
    if n and (int(labels.shape[0]) != n or _np_dtype(labels) != np.dtype(np.int32)):
        raise RuntimeError("KokkosGraph::graph_explicit_coarsen: labels must hold num_verts int32 entries")
    crm = be.empty(nc + 1, _np_dtype(row_map))
    inv_off = be.empty(nc + 1, np.int32) if inverse_map else None
    inv_lab = be.empty(max(n, 1), np.int32) if inverse_map else None
    nnz = C.c_int64()
    room = int(entries.shape[0])
    cent = be.empty(max(room, 1), np.int32)
    check(lib, lib.kkamd_graph_explicit_coarsen(n, be.ptr(row_map), _offset_type(row_map), be.ptr(entries), be.ptr(labels), nc, 1 if compress else 0,
                                                be.ptr(crm), be.ptr(cent), room, C.byref(nnz), be.ptr(inv_off), be.ptr(inv_lab), be.stream()))
    if inverse_map:
        return crm, cent[:nnz.value], inv_off, inv_lab[:n]
    return crm, cent[:nnz.value]


def sort_crs_matrix(A):
    be, lib = A.backend, A.backend.lib
    check(lib, lib.kkamd_sort_crs(A.numRows(), be.ptr(A.graph.row_map), be.ptr(A.graph.entries),
                                  be.ptr(A.values) if A.values is not None else None,
                                  _offset_type(A.graph.row_map), _scalar_type(A.values) if A.values is not None else F64,
                                  be.stream()))
    return A


def sort_and_merge_matrix(A):
    """KokkosSparse::sort_and_merge_matrix (sparse/src/KokkosSparse_SortCrs.hpp:304-400): returns a new matrix whose rows
    are sorted with duplicate columns summed; A itself is left sorted (as in the reference, which sorts its input views)."""
    be, lib = A.backend, A.backend.lib
    m = A.numRows()
    rm_out = be.empty(m + 1, _np_dtype(A.graph.row_map))
    ot = _offset_type(A.graph.row_map)
    vt = _scalar_type(A.values) if A.values is not None else F64
    n = C.c_int64()
    vals = be.ptr(A.values) if A.values is not None else None
    check(lib, lib.kkamd_sort_and_merge(m, be.ptr(A.graph.row_map), be.ptr(A.graph.entries), vals, ot, vt, be.ptr(rm_out), None, None,
                                        C.byref(n), be.stream()))
    ent = be.empty(max(n.value, 1), np.int32)
    val = be.empty(max(n.value, 1), _np_dtype(A.values)) if A.values is not None else None
    check(lib, lib.kkamd_sort_and_merge(m, be.ptr(A.graph.row_map), be.ptr(A.graph.entries), vals, ot, vt, be.ptr(rm_out), be.ptr(ent),
                                        be.ptr(val) if val is not None else None, C.byref(n), be.stream()))
    return CrsMatrix(m, A.numCols(), rm_out, ent[:n.value], val[:n.value] if val is not None else None, backend=be)


def transpose_matrix(A):
    """KokkosSparse::Impl::transpose_matrix (sparse/src/KokkosSparse_Utils.hpp:381-398); rows of the result are sorted."""
    be, lib = A.backend, A.backend.lib
    m, n, nnz = A.numRows(), A.numCols(), A.nnz()
    t_rm = be.empty(n + 1, _np_dtype(A.graph.row_map))
    t_ent = be.empty(max(nnz, 1), np.int32)
    t_val = be.empty(max(nnz, 1), _np_dtype(A.values)) if A.values is not None else None
    check(lib, lib.kkamd_transpose(m, n, nnz, be.ptr(A.graph.row_map), be.ptr(A.graph.entries),
                                   be.ptr(A.values) if A.values is not None else None, _offset_type(A.graph.row_map),
                                   _scalar_type(A.values) if A.values is not None else F64, be.ptr(t_rm), be.ptr(t_ent),
                                   be.ptr(t_val) if t_val is not None else None, be.stream()))
    return CrsMatrix(n, m, t_rm, t_ent[:nnz], t_val[:nnz] if t_val is not None else None, backend=be)


def laplace_matrix(stencil, nx, ny, nz=None, offset_dtype=np.int32, value_dtype=np.float64, backend=None, rows=None):
    """Structured Laplacian (every BC = 1) generated in place on the device; bit-identical to the
    reference's generate_structured_matrix2D/3D (test_common/KokkosKernels_Test_Structured_Matrix.hpp).
    rows=(begin, count) builds only that row slab (local row_map, global columns)."""
    be = backend or torch_backend()
    lib = be.lib
    dim = 2 if nz is None else 3
    s = {"FD": 0, "FE": 1}[stencil]
    n = nx * ny * (nz or 1)
    r0, cnt = rows if rows is not None else (0, n)
    rm = be.empty(cnt + 1, offset_dtype)
    nnz = C.c_int64()
    ot = I64 if np.dtype(offset_dtype) == np.dtype(np.int64) else I32
    vt = F64 if np.dtype(value_dtype) == np.dtype(np.float64) else F32
    check(lib, lib.kkamd_gen_laplace_rows(dim, s, nx, ny, nz or 1, r0, cnt, be.ptr(rm), None, None, ot, vt, C.byref(nnz),
                                          be.stream()))
    ent = be.empty(nnz.value, np.int32)
    val = be.empty(nnz.value, value_dtype)
    check(lib, lib.kkamd_gen_laplace_rows(dim, s, nx, ny, nz or 1, r0, cnt, be.ptr(rm), be.ptr(ent), be.ptr(val), ot, vt,
                                          C.byref(nnz), be.stream()))
    return CrsMatrix(cnt, n, rm, ent, val, backend=be)
