"""ctypes signatures of libkkamd.so (include/kkamd.h).  Pointer plumbing only: every compute call
goes to the HIP library; there is no Python or CPU implementation behind these functions."""
import ctypes as C

F32, F64 = 0, 1
I32, I64 = 0, 1
OK, ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_HIP, ERR_ALLOC, ERR_STATE = range(6)
ERR_NUMERIC = 6
SPMV_DEFAULT, SPMV_FAST_SETUP, SPMV_NATIVE, SPMV_MERGE_PATH, SPMV_NATIVE_MERGE_PATH = range(5)
SPTRSV_SEQLVLSCHD_RP, SPTRSV_SEQLVLSCHD_TP1, SPTRSV_SEQLVLSCHD_TP1CHAIN, SPTRSV_CUSPARSE = range(4)
SPILUK_SEQLVLSCHD_TP1 = 0

EXPORTS = [
    "kkamd_last_error", "kkamd_version", "kkamd_device_info", "kkamd_trace_push", "kkamd_trace_pop", "kkamd_spmv_plan_create", "kkamd_spmv_plan_create_knobs", "kkamd_release_scratch", "kkamd_spmv_plan_destroy",
    "kkamd_spmv", "kkamd_spmv_mv", "kkamd_spmv_struct", "kkamd_sort_and_merge", "kkamd_transpose", "kkamd_spmv_plan_set", "kkamd_spmv_plan_values_changed", "kkamd_spmv_plan_query", "kkamd_spmv_plan_export", "kkamd_set_default", "kkamd_spgemm_create",
    "kkamd_spgemm_destroy", "kkamd_spgemm_set", "kkamd_spgemm_symbolic", "kkamd_spgemm_numeric", "kkamd_spgemm_jacobi", "kkamd_spgemm_get", "kkamd_spgemm_get_hint", "kkamd_sort_crs",
    "kkamd_exclusive_scan", "kkamd_gen_laplace", "kkamd_gen_laplace_rows", "kkamd_bench_read",
    "kkamd_dist_unique_id", "kkamd_dist_transport_selftest", "kkamd_dist_spmv_create", "kkamd_dist_spmv_destroy", "kkamd_dist_spmv_x_local", "kkamd_dist_spmv_apply",
    "kkamd_dist_spmv_query",
    "kkamd_dist_spgemm_partition", "kkamd_dist_spgemm_create", "kkamd_dist_spgemm_destroy", "kkamd_dist_spgemm_handle", "kkamd_dist_spgemm_symbolic",
    "kkamd_dist_spgemm_numeric", "kkamd_dist_spgemm_jacobi", "kkamd_dist_spgemm_query",
]
# the sparse triangular solve: bound when the loaded library exports it (the emulator library of tests/emu/Makefile does not)
SPTRSV_EXPORTS = ["kkamd_sptrsv_create", "kkamd_sptrsv_destroy", "kkamd_sptrsv_symbolic", "kkamd_sptrsv_solve", "kkamd_sptrsv_set",
                  "kkamd_sptrsv_get", "kkamd_sptrsv_export"]
# ILU(k): bound when the loaded library exports it, like the triangular solve
SPILUK_EXPORTS = ["kkamd_spiluk_create", "kkamd_spiluk_destroy", "kkamd_spiluk_symbolic", "kkamd_spiluk_numeric", "kkamd_spiluk_set",
                  "kkamd_spiluk_get", "kkamd_spiluk_export"]
# multicolor Gauss-Seidel: bound when the loaded library exports it, like the triangular solve
GS_EXPORTS = ["kkamd_gs_create", "kkamd_gs_destroy", "kkamd_gs_symbolic", "kkamd_gs_numeric", "kkamd_gs_apply", "kkamd_gs_set", "kkamd_gs_get",
              "kkamd_gs_export"]
GS_DEFAULT, GS_PERMUTED, GS_TEAM, GS_CLUSTER, GS_TWOSTAGE = range(5)
# restarted GMRES and the preconditioners: bound when the loaded library exports them, like the triangular solve
GMRES_EXPORTS = ["kkamd_gmres_create", "kkamd_gmres_destroy", "kkamd_gmres_set", "kkamd_gmres_set_tol", "kkamd_gmres_reset", "kkamd_gmres_get",
                 "kkamd_gmres_get_real", "kkamd_gmres_export", "kkamd_gmres_solve", "kkamd_gmres_dot", "kkamd_gmres_update",
                 "kkamd_precond_create_matrix", "kkamd_precond_create_lu", "kkamd_precond_create_callback", "kkamd_precond_apply",
                 "kkamd_precond_destroy"]
GMRES_CGS2, GMRES_MGS = range(2)
GMRES_CONV, GMRES_NO_CONV, GMRES_LOA, GMRES_NOT_RUN = range(4)
GS_FORWARD, GS_BACKWARD, GS_SYMMETRIC = range(3)
# ParILUT: bound when the loaded library exports it, like the triangular solve
PAR_ILUT_EXPORTS = ["kkamd_par_ilut_create", "kkamd_par_ilut_destroy", "kkamd_par_ilut_symbolic", "kkamd_par_ilut_numeric",
                    "kkamd_par_ilut_copy_factors", "kkamd_par_ilut_set", "kkamd_par_ilut_get", "kkamd_par_ilut_get_real",
                    "kkamd_par_ilut_add_candidates", "kkamd_par_ilut_sweep", "kkamd_par_ilut_select", "kkamd_par_ilut_filter",
                    "kkamd_par_ilut_residual"]
# MIS-2, aggregation, explicit coarsening: bound when the loaded library exports them, like the triangular solve
MIS2_EXPORTS = ["kkamd_graph_d2_mis", "kkamd_graph_mis2_aggregate", "kkamd_graph_explicit_coarsen"]
MIS2_QUALITY, MIS2_FAST = range(2)

ALL_GATHER_FN =C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int), C.c_int,
                          C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int), C.c_void_p)


# kkamd_precond_fn: (ctx, d_x, d_y, alpha, beta, value_type, stream) -> status
PRECOND_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p)


class Transport(C.Structure):
    """kkamd_transport_t: how the multi-GPU SpMV moves x entries when it is not the built-in RCCL"""
    _fields_ = [("ctx", C.c_void_p), ("all_gather", ALL_GATHER_FN), ("exchange", EXCHANGE_FN)]


class CrsDesc(C.Structure):
    _fields_ = [("num_rows", C.c_int64), ("num_cols", C.c_int64), ("nnz", C.c_int64), ("d_row_map", C.c_void_p),
                ("d_entries", C.c_void_p), ("d_values", C.c_void_p), ("offset_type", C.c_int), ("value_type", C.c_int)]


class KkamdError(RuntimeError):
    """Non-zero kkamd_status.  .status holds the code; the C++ shim maps INVALID_ARG/HIP to
    std::runtime_error and STATE to std::invalid_argument like the reference."""

    def __init__(self, status, msg):
        super().__init__("kkamd status %d: %s" % (status, msg))
        self.status = status


def bind(lib):
    vp, i64, ci, dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
    lib.kkamd_last_error.restype = C.c_char_p
    lib.kkamd_version.restype = ci
    lib.kkamd_device_info.argtypes = [C.c_char_p, ci, C.POINTER(ci), C.POINTER(ci)]
    lib.kkamd_trace_push.argtypes = [C.c_char_p]
    lib.kkamd_trace_pop.argtypes = []
    lib.kkamd_spmv_plan_create.argtypes = [C.POINTER(vp), C.POINTER(CrsDesc), ci, vp]
    lib.kkamd_spmv_plan_create_knobs.argtypes = [C.POINTER(vp), C.POINTER(CrsDesc), ci, C.POINTER(C.c_char_p), C.POINTER(ci), ci, vp]
    lib.kkamd_release_scratch.argtypes = []
    lib.kkamd_spmv_plan_destroy.argtypes = [vp]
    lib.kkamd_spmv.argtypes = [vp, C.POINTER(CrsDesc), C.c_char, dbl, vp, dbl, vp, ci, vp]
    lib.kkamd_spmv_mv.argtypes = [vp, C.POINTER(CrsDesc), C.c_char, dbl, vp, i64, i64, dbl, vp, i64, i64, i64, ci, vp]
    lib.kkamd_spmv_struct.argtypes = [C.POINTER(CrsDesc), C.c_char, ci, ci, C.POINTER(i64), dbl, vp, dbl, vp, ci, vp]
    lib.kkamd_spmv_plan_set.argtypes = [vp, C.c_char_p, ci]
    lib.kkamd_spmv_plan_values_changed.argtypes = [vp]
    lib.kkamd_set_default.argtypes = [C.c_char_p, ci]
    lib.kkamd_spmv_plan_query.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
    lib.kkamd_spmv_plan_export.argtypes = [vp, C.c_char_p, vp, i64]
    lib.kkamd_spgemm_create.argtypes = [C.POINTER(vp)]
    lib.kkamd_spgemm_destroy.argtypes = [vp]
    lib.kkamd_spgemm_set.argtypes = [vp, C.c_char_p, dbl]
    lib.kkamd_spgemm_symbolic.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, ci, C.POINTER(i64), vp]
    lib.kkamd_spgemm_numeric.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]
    lib.kkamd_spgemm_jacobi.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, dbl, vp, ci, ci, vp]
    lib.kkamd_spgemm_get.argtypes = [vp, ci, C.POINTER(i64)]
    lib.kkamd_spgemm_get_hint.argtypes = [vp, C.c_char_p, C.POINTER(dbl)]
    lib.kkamd_sort_crs.argtypes = [i64, vp, vp, vp, ci, ci, vp]
    lib.kkamd_exclusive_scan.argtypes = [vp, i64, ci, vp]
    lib.kkamd_sort_and_merge.argtypes = [i64, vp, vp, vp, ci, ci, vp, vp, vp, C.POINTER(i64), vp]
    lib.kkamd_transpose.argtypes = [i64, i64, i64, vp, vp, vp, ci, ci, vp, vp, vp, vp]
    lib.kkamd_gen_laplace.argtypes = [ci, ci, i64, i64, i64, vp, vp, vp, ci, ci, C.POINTER(i64), vp]
    lib.kkamd_gen_laplace_rows.argtypes = [ci, ci, i64, i64, i64, i64, i64, vp, vp, vp, ci, ci, C.POINTER(i64), vp]
    lib.kkamd_bench_read.argtypes = [vp, i64, ci, ci, ci, vp, vp]
    lib.kkamd_dist_unique_id.argtypes = [vp]
    lib.kkamd_dist_transport_selftest.argtypes = [i64, vp]
    lib.kkamd_dist_spmv_create.argtypes = [C.POINTER(vp), C.POINTER(CrsDesc), C.POINTER(i64), ci, ci, vp, C.POINTER(Transport), ci, ci, ci, ci, vp]
    lib.kkamd_dist_spmv_destroy.argtypes = [vp]
    lib.kkamd_dist_spmv_x_local.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    lib.kkamd_dist_spmv_apply.argtypes = [vp, dbl, vp, dbl, vp, ci, vp]
    lib.kkamd_dist_spmv_query.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
    lib.kkamd_dist_spgemm_partition.argtypes = [i64, vp, vp, vp, ci, ci, C.POINTER(i64), C.POINTER(i64), vp]
    lib.kkamd_dist_spgemm_create.argtypes = [C.POINTER(vp), ci, ci, C.POINTER(i64)]
    lib.kkamd_dist_spgemm_destroy.argtypes = [vp]
    lib.kkamd_dist_spgemm_handle.argtypes = [vp]
    lib.kkamd_dist_spgemm_symbolic.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, ci, C.POINTER(i64), vp]
    lib.kkamd_dist_spgemm_numeric.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]
    lib.kkamd_dist_spgemm_jacobi.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, dbl, vp, ci, ci, vp]
    lib.kkamd_dist_spgemm_query.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
    names = list(EXPORTS)
    if hasattr(lib, "kkamd_sptrsv_create"):
        lib.kkamd_sptrsv_create.argtypes = [C.POINTER(vp), ci, i64, ci]
        lib.kkamd_sptrsv_destroy.argtypes = [vp]
        lib.kkamd_sptrsv_symbolic.argtypes = [vp, i64, vp, vp, ci, vp]
        lib.kkamd_sptrsv_solve.argtypes = [vp, i64, vp, vp, vp, vp, vp, ci, ci, vp]
        lib.kkamd_sptrsv_set.argtypes = [vp, C.c_char_p, ci]
        lib.kkamd_sptrsv_get.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
        lib.kkamd_sptrsv_export.argtypes = [vp, C.c_char_p, vp, i64]
        names += SPTRSV_EXPORTS
    if hasattr(lib, "kkamd_spiluk_create"):
        lib.kkamd_spiluk_create.argtypes = [C.POINTER(vp), ci, i64, i64, i64]
        lib.kkamd_spiluk_destroy.argtypes = [vp]
        lib.kkamd_spiluk_symbolic.argtypes = [vp, ci, i64, vp, vp, vp, vp, i64, vp, vp, i64, ci, vp]
        lib.kkamd_spiluk_numeric.argtypes = [vp, ci, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci, vp]
        lib.kkamd_spiluk_set.argtypes = [vp, C.c_char_p, ci]
        lib.kkamd_spiluk_get.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
        lib.kkamd_spiluk_export.argtypes = [vp, C.c_char_p, vp, i64]
        names += SPILUK_EXPORTS
    if hasattr(lib, "kkamd_gs_create"):
        lib.kkamd_gs_create.argtypes = [C.POINTER(vp), ci]
        lib.kkamd_gs_destroy.argtypes = [vp]
        lib.kkamd_gs_symbolic.argtypes = [vp, i64, i64, vp, vp, ci, ci, vp, vp]
        lib.kkamd_gs_numeric.argtypes = [vp, i64, i64, vp, vp, vp, vp, ci, ci, vp]
        lib.kkamd_gs_apply.argtypes = [vp, i64, i64, vp, vp, vp, vp, i64, i64, vp, i64, i64, i64, ci, ci, dbl, ci, ci, ci, ci, vp]
        lib.kkamd_gs_set.argtypes = [vp, C.c_char_p, ci]
        lib.kkamd_gs_get.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
        lib.kkamd_gs_export.argtypes = [vp, C.c_char_p, vp, i64]
        names += GS_EXPORTS
    if hasattr(lib, "kkamd_gmres_create"):
        lib.kkamd_gmres_create.argtypes = [C.POINTER(vp), i64, dbl, i64]
        lib.kkamd_gmres_destroy.argtypes = [vp]
        lib.kkamd_gmres_set.argtypes = [vp, C.c_char_p, i64]
        lib.kkamd_gmres_set_tol.argtypes = [vp, dbl]
        lib.kkamd_gmres_reset.argtypes = [vp, i64, dbl, i64]
        lib.kkamd_gmres_get.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
        lib.kkamd_gmres_get_real.argtypes = [vp, C.c_char_p, C.POINTER(dbl)]
        lib.kkamd_gmres_export.argtypes = [vp, C.c_char_p, vp, i64]
        lib.kkamd_gmres_solve.argtypes = [vp, C.POINTER(CrsDesc), vp, vp, vp, ci, vp]
        lib.kkamd_gmres_dot.argtypes = [vp, i64, i64, vp, i64, vp, vp, ci, vp]
        lib.kkamd_gmres_update.argtypes = [vp, i64, i64, dbl, vp, i64, vp, vp, vp, vp, vp, ci, vp]
        lib.kkamd_precond_create_matrix.argtypes = [C.POINTER(vp), C.POINTER(CrsDesc), vp]
        lib.kkamd_precond_create_lu.argtypes = [C.POINTER(vp), C.POINTER(CrsDesc), C.POINTER(CrsDesc), vp]
        lib.kkamd_precond_create_callback.argtypes = [C.POINTER(vp), PRECOND_FN, vp]
        lib.kkamd_precond_apply.argtypes = [vp, vp, vp, dbl, dbl, ci, vp]
        lib.kkamd_precond_destroy.argtypes = [vp]
        names += GMRES_EXPORTS
    if hasattr(lib, "kkamd_par_ilut_create"):
        lib.kkamd_par_ilut_create.argtypes = [C.POINTER(vp), i64, dbl, dbl, ci, ci]
        lib.kkamd_par_ilut_destroy.argtypes = [vp]
        lib.kkamd_par_ilut_symbolic.argtypes = [vp, i64, vp, vp, vp, vp, ci, vp]
        lib.kkamd_par_ilut_numeric.argtypes = [vp, i64, vp, vp, vp, vp, vp, ci, ci, vp]
        lib.kkamd_par_ilut_copy_factors.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp]
        lib.kkamd_par_ilut_set.argtypes = [vp, C.c_char_p, dbl]
        lib.kkamd_par_ilut_get.argtypes = [vp, C.c_char_p, C.POINTER(i64)]
        lib.kkamd_par_ilut_get_real.argtypes = [vp, C.c_char_p, C.POINTER(dbl)]
        lib.kkamd_par_ilut_add_candidates.argtypes = [vp, i64] + [vp] * 12 + [i64, vp, vp, vp, i64, vp, vp, vp, i64, C.POINTER(i64), C.POINTER(i64), ci, ci, vp]
        lib.kkamd_par_ilut_sweep.argtypes = [vp, i64] + [vp] * 12 + [ci, ci, vp]
        lib.kkamd_par_ilut_select.argtypes = [vp, i64, vp, i64, vp, ci, vp]
        lib.kkamd_par_ilut_filter.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, C.POINTER(i64), ci, ci, vp]
        lib.kkamd_par_ilut_residual.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, C.POINTER(dbl), ci, ci, vp]
        names += PAR_ILUT_EXPORTS
    if hasattr(lib, "kkamd_graph_d2_mis"):
        lib.kkamd_graph_d2_mis.argtypes = [i64, vp, ci, vp, ci, vp, C.POINTER(i64), C.POINTER(i64), vp]
        lib.kkamd_graph_mis2_aggregate.argtypes = [i64, vp, ci, vp, ci, vp, C.POINTER(i64), C.POINTER(i64), vp]
        lib.kkamd_graph_explicit_coarsen.argtypes = [i64, vp, ci, vp, vp, i64, ci, vp, vp, i64, C.POINTER(i64), vp, vp, vp]
        names += MIS2_EXPORTS
    for name in names:
        fn = getattr(lib, name)
        if name == "kkamd_dist_spgemm_handle":
            fn.restype = vp
        elif name not in ("kkamd_last_error",):
            fn.restype = ci
    return lib


def check(lib, status):
    if status != OK:
        raise KkamdError(status, lib.kkamd_last_error().decode(errors="replace"))
