/* kkamd.h -- C ABI of libkkamd.so: the MI355X (gfx950) native implementation of the
 * KokkosSparse::spmv / KokkosSparse::spgemm / KokkosSparse::sptrsv / KokkosSparse::spiluk / KokkosSparse::gauss_seidel /
 * KokkosSparse::Experimental::gmres hot path.
 *
 * This is the drop-in boundary.  It sits exactly where kokkos-kernels plugs vendor libraries in
 * today -- the "TPL specialisation" layer -- and takes what those specialisations hand over:
 * raw device pointers unwrapped from Kokkos::Views, extents, and the execution-space instance's
 * HIP stream.  Each entry point cites the reference interface it replaces (paths relative to the
 * kokkos-kernels 4.7.00 tree).  INTEGRATION.md shows the *_tpl_spec_{avail,decl}.hpp siblings a
 * maintainer adds on the reference side to bind them.
 *
 * Conventions
 *   - plain C, no C++/torch/Kokkos types; every pointer named d_* is a DEVICE pointer, borrowed
 *     for the duration of the call (the reference's Unmanaged views);
 *   - every function returns a kkamd_status (0 = ok) and never throws; kkamd_last_error() gives the
 *     message for the calling thread.  The C++ shim turns non-zero into the exception type the
 *     reference would throw (std::runtime_error / std::invalid_argument);
 *   - kkamd_stream_t is hipStream_t (a pointer to the opaque ihipStream_t); SpMV entry points are
 *     asynchronous on that stream, SpGEMM phases synchronise it where they must return counts;
 *   - CSR: zero-based, row_map has num_rows+1 offsets (int32 or int64), entries are int32 ordinals
 *     (the reference requires a signed ordinal: sparse/src/KokkosSparse_CrsMatrix.hpp:320),
 *     values float or double.
 */
#ifndef KKAMD_H
#define KKAMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KKAMD_VERSION 100

typedef struct ihipStream_t* kkamd_stream_t;

typedef enum {
  KKAMD_OK               = 0,
  KKAMD_ERR_INVALID_ARG  = 1, /* dimension/type/pointer problems (reference: std::runtime_error)        */
  KKAMD_ERR_UNSUPPORTED  = 2, /* type tuple or mode not implemented here: caller diverts to native path  */
  KKAMD_ERR_HIP          = 3, /* a HIP runtime call failed (reference: *_SAFE_CALL -> std::runtime_error)*/
  KKAMD_ERR_ALLOC        = 4,
  KKAMD_ERR_STATE        = 5, /* handle misuse, e.g. numeric before symbolic (std::invalid_argument)    */
  KKAMD_ERR_NUMERIC      = 6  /* a solver stopped on its numbers: GMRES breakdown, NaN residual (std::runtime_error) */
} kkamd_status;

typedef enum { KKAMD_F32 = 0, KKAMD_F64 = 1 } kkamd_scalar_type;
typedef enum { KKAMD_I32 = 0, KKAMD_I64 = 1 } kkamd_offset_type;

/* KokkosSparse::SPMVAlgorithm (sparse/src/KokkosSparse_spmv_handle.hpp:32-47), CRS subset. */
typedef enum {
  KKAMD_SPMV_DEFAULT           = 0,
  KKAMD_SPMV_FAST_SETUP        = 1,
  KKAMD_SPMV_NATIVE            = 2,
  KKAMD_SPMV_MERGE_PATH        = 3,
  KKAMD_SPMV_NATIVE_MERGE_PATH = 4
} kkamd_spmv_algorithm;

/* CrsMatrix as the TPL layer sees it: (numRows, numCols, nnz, graph.row_map.data(),
 * graph.entries.data(), values.data()) -- sparse/tpls/KokkosSparse_spmv_tpl_spec_decl.hpp:332-338. */
typedef struct {
  int64_t num_rows;
  int64_t num_cols;
  int64_t nnz;
  const void* d_row_map; /* offset_type[num_rows + 1] */
  const void* d_entries; /* int32_t[nnz]              */
  const void* d_values;  /* value_type[nnz]           */
  int offset_type;       /* kkamd_offset_type         */
  int value_type;        /* kkamd_scalar_type         */
} kkamd_crs_t;

const char* kkamd_last_error(void);
int kkamd_version(void);
/* Profiling ranges (roctx, shown by rocprofv3 --marker-trace): what Kokkos::Profiling::pushRegion / popRegion map to on the
 * host side of the boundary.  The library's own entry points open ranges labelled like the reference's
 * ("KokkosSparse::spmv[TPL_KKAMD,double]", sparse/tpls/KokkosSparse_spmv_tpl_spec_decl.hpp:411-414). */
int kkamd_trace_push(const char* label);
int kkamd_trace_pop(void);
/* name of the device the library is running on and whether it is gfx950; used by tests. */
int kkamd_device_info(char* name, int name_len, int* is_gfx950, int* num_cus);

/* ------------------------------------------------------------------------------------------------
 * SpMV.  Replaces Impl::SPMV<Kokkos::HIP,...>::spmv and Impl::SPMV_MV<...>::spmv_mv
 * (sparse/impl/KokkosSparse_spmv_spec.hpp:92-135; vendor precedent
 * sparse/tpls/KokkosSparse_spmv_tpl_spec_decl.hpp:278-425 and ..._spmv_mv_tpl_spec_decl.hpp:284-430).
 *
 * A plan is the analogue of SPMVHandleImpl::tpl_rank1 / tpl_rank2
 * (sparse/src/KokkosSparse_spmv_handle.hpp:241-242): created lazily on the first call with a handle,
 * bound to ONE matrix for life (:273-277), destroyed with the handle.  plan == NULL is the
 * handle-less / SPMV_FAST_SETUP route: no analysis, no workspace.
 * ------------------------------------------------------------------------------------------------ */
typedef struct kkamd_spmv_plan kkamd_spmv_plan_t;

int kkamd_spmv_plan_create(kkamd_spmv_plan_t** plan, const kkamd_crs_t* A, int algorithm, kkamd_stream_t stream);
/* same, with this plan's expert knobs (see kkamd_spmv_plan_set) applied BEFORE the analysis they shape; the library-wide
 * defaults are not touched. */
int kkamd_spmv_plan_create_knobs(kkamd_spmv_plan_t** plan, const kkamd_crs_t* A, int algorithm, const char* const* keys,
                                 const int* values, int nknobs, kkamd_stream_t stream);
int kkamd_spmv_plan_destroy(kkamd_spmv_plan_t* plan);
/* Frees the calling host thread's scratch of the handle-less route (tile descriptors + carry slots, grown on demand and
 * otherwise kept for the thread's life) and the two process-wide buffers of the SpGEMM symbolic phase: the store of the structure it
 * keeps for the first numeric call (bitmaps and entry lists of the dense class's units: at most 0.225 of the free HBM, or
 * "spgemm_store_cap_mb") and the phase's temporaries (the two indices and the units' products: 0.7 GB at R-MAT scale 20); also the
 * 512-byte counter blocks (device + pinned host) that destroyed SpGEMM handles leave for the next handle.  The two large buffers are
 * kept between uses under the policy of "spgemm_pool_keep" because allocating and freeing GBs per handle costs more than the phase
 * itself. */
int kkamd_release_scratch(void);

/* y := alpha*op(A)*x + beta*y.  mode 'N','C' (== 'N' for real scalars), 'T','H' (== 'T').
 * vector_type is the scalar type of x and y (and of alpha/beta, the reference's coefficient_type);
 * supported (value_type, vector_type) pairs: (F64,F64), (F32,F32), (F32,F64).
 * beta == 0 overwrites y (NaN/Inf in the old y are discarded: sparse/src/KokkosSparse_spmv.hpp:145-154,
 * sparse/impl/KokkosSparse_spmv_impl.hpp:127-131).  alpha == 0 / empty A reduce to the y scaling. */
int kkamd_spmv(kkamd_spmv_plan_t* plan, const kkamd_crs_t* A, char mode, double alpha, const void* d_x, double beta,
               void* d_y, int vector_type, kkamd_stream_t stream);

/* Rank-2: X is (num_cols x nvec), Y is (num_rows x nvec) for 'N'; element (i,j) lives at
 * i*stride0 + j*stride1 (in elements), which covers LayoutLeft (1, ld), LayoutRight (ld, 1) and the
 * mixed pairs the rocSPARSE plug-in accepts (sparse/tpls/KokkosSparse_spmv_mv_tpl_spec_avail.hpp:108-134). */
int kkamd_spmv_mv(kkamd_spmv_plan_t* plan, const kkamd_crs_t* A, char mode, double alpha, const void* d_X,
                  int64_t x_stride0, int64_t x_stride1, double beta, void* d_Y, int64_t y_stride0, int64_t y_stride1,
                  int64_t nvec, int vector_type, kkamd_stream_t stream);

/* KokkosSparse::Experimental::spmv_struct (sparse/src/KokkosSparse_spmv.hpp:478-559, impl
 * sparse/impl/KokkosSparse_spmv_struct_impl.hpp:640-705): y := alpha*op(A)*x + beta*y for a matrix that comes from a
 * 3-pt (1-D), 5-/9-pt (2-D, stencil_type 1 = FD / 2 = FE) or 7-/27-pt (3-D) stencil on a structure[0] x structure[1] x
 * structure[2] grid, rows numbered i fastest.  Interior rows never read entries(): their idx-th value multiplies
 * x(row + offset(idx)); exterior rows take the CRS row.  y is not read when beta == 0 (BLAS convention; the reference's
 * functor evaluates beta*y + alpha*sum also then) and modes 'T'/'H' ignore the structure.  structure is a HOST array of ndim extents. */
int kkamd_spmv_struct(const kkamd_crs_t* A, char mode, int stencil_type, int ndim, const int64_t* structure, double alpha,
                      const void* d_x, double beta, void* d_y, int vector_type, kkamd_stream_t stream);

/* Expert knobs, the analogue of SPMVHandleImpl's public tuning members
 * (sparse/src/KokkosSparse_spmv_handle.hpp:243-252); per plan (kkamd_spmv_plan_set / kkamd_spmv_plan_create_knobs), or as
 * defaults for plans created later (kkamd_set_default).  Values outside the listed ranges return KKAMD_ERR_INVALID_ARG.
 *   SpMV, rank 1
 *     "kernel"          0 auto, 1 no-analysis vector kernel, 2 nnz-split kernel
 *     "lanes_per_row"   vector kernel, 0 = from nnz / row (the reference's vector_length)
 *     "nnz_per_thread"  nnz-split kernel: 4 (fp64 values only) | 8 | 16 nonzeros per work-item = 1024 / 2048 / 4096 per tile, 0 = by size
 *     "xcd_remap"       tile order: 0 dispatch, 1 XCD-contiguous, 2^k grouped (default 16)
 *     "window_codes"    per-tile column analysis of an analysed handle: 1 (default) 16-bit window codes + LDS-staged x where a tile's
 *                       columns allow it, 2 codes without staged x, 0 never; from "window_codes_min_knnz" thousand nonzeros and when
 *                       at least "window_codes_min_pct" percent of the tiles can use them (the others read entries, tile by tile);
 *                       "stream_variant" 6 attempts the analysis whatever the size (tests), 1 is the default
 *     "pattern_codes"   staged-x tiles: row-pattern records instead of per-nonzero codes; 1 (default) when >= 90 % of the tiles
 *                       decompose, 2 whenever one does, 0 never; from "pattern_codes_min_knnz" thousand nonzeros.  "pattern_direct" 1
 *                       (default): the records are first sought straight in the matrix (rows compared, the window cover over the <= 256
 *                       column intervals of a tile) and kept when at most one tile in a hundred has none -- those read entries --, no
 *                       window codes are built (plan of 27-pt 300^3: 6.2 -> 2.5 ms); 0: always by way of the codes.  Query "pattern_direct"
 *     "transient_min_knnz"  handle-less / FAST_SETUP calls analyse on the fly from this many thousand nonzeros (0 never)
 *     "explicit_transpose"  modes T/H with an analysed handle (rank 1 and rank 2): 1 (default) through a transpose cached in the plan when
 *                       it fits an eighth of free HBM, its values follow "values_tracking"; 2 the caller promises constant
 *                       values (no tracking pass either); 0 the reference's atomic scatter.  From "explicit_transpose_min_knnz"
 *     "values_tracking" how a re-ordered copy of A.values (cached transpose; column-slab copy) follows value changes: 0 (default) EXACT --
 *                       a shadow copy of A.values in A's order, compared bit for bit at every call (two streams of 8 B per nonzero),
 *                       changed 4096-value tiles are moved; without memory for the shadow every call copies all values; 1 NOTIFY --
 *                       kkamd_spmv_plan_values_changed says when, nothing is read in between; 2 FINGERPRINTS -- 128 bits per tile, one
 *                       stream, no shadow: a heuristic (a changed tile with an unchanged fingerprint is missed)
 *     "check_entries"   debug aid, 0 (default) / 1: every call hashes the matrix's column array (one pass + a stream synchronisation) and
 *                       returns KKAMD_ERR_STATE when it differs from what the handle first saw: a structure edited in place under a live
 *                       handle (the pointer comparison of every call cannot see that; rocSPARSE's analysis has the same contract)
 *     "colslab"         mode N on matrices whose x gather defeats the caches (most tiles read plain entries, x is >= 16 MB, from
 *                       "colslab_min_knnz" thousand nonzeros): a second copy of the matrix in column-slab order (entries sorted by 2 MB
 *                       segments of x, then by row; nnz * (8 + value + offset) bytes) whose values follow "values_tracking".
 *                       3 (default): the DETERMINISTIC form -- per-slab partial sums of every row with one writer each, slabs added in
 *                       ascending order: no atomics, the same bits on every run --, chosen at the first call by a RULE, nothing is timed:
 *                       sampled windows of the matrix name at least "colslab_min_pct" (85) percent of a 128-byte line of x per nonzero,
 *                       and the bytes the slab form streams, priced at "colslab_rate_pct" (61: its rate over the rate at which the CRS
 *                       kernel's gathers pull lines, 4.24 / 6.95 TB/s measured on MI355X) of the lines the CRS kernel would pull, are
 *                       fewer by 10 %; 4 always the deterministic form (tests); 1 the ATOMIC form (products reach y through atomics:
 *                       results agree with the CRS kernel to rounding and vary in the last bits from run to run), chosen by timing both
 *                       kernels ON THE CALLER'S STREAM inside the first call (the call blocks), kept when 10 % faster; 2 always the
 *                       atomic form (tests); 0 never.  "colslab_shift" log2 of the columns per slab (0 = automatic),
 *                       "colslab_const" 1 = the caller promises constant matrix values (no tracking pass)
 *   SpMV, rank 2
 *     "mv6"             nonzero-split kernel (kk_spmv_mvnnz.hip; analysed plan, fp64 vectors): the nonzeros are cut into chunks of 128 per
 *                       16-lane group, the plan keeps the row index of every nonzero (4 B per nonzero), rows cut by a chunk boundary are
 *                       finished from carry slots (no atomics, deterministic).  1 (default) on matrices with at least
 *                       "mv6_min_long_pct" (10) percent of their nonzeros in rows above 4 x the average length (at least 64): power-law
 *                       graphs; 2 whenever the gather kernel would run; 0 never
 *     "mv_kernel"       0 auto (plane-marching kernel where it applies -- analysed plan, fp64 vectors, right-hand sides in
 *                       blocks of 16 (a remainder: one more pass over the last 16 columns when beta = 0, else the gather kernel), a matrix that verifies as a radius-1 lattice stencil --, else the wave-private gather
 *                       kernel), 1 generic strided kernel, 2 wave-private gather kernel, 3 LDS-staged X tiles, 4 = 0 without the matrix-core
 *                       kernel, 5 = 0 (the matrix-core kernel where its analysis accepts the matrix, see "mv5"), 6 = the nonzero-split or the gather kernel
 *     "mv5"             matrix-core kernel (v_mfma_f64_16x16x4f64; analysed plan, fp64 vectors, any width and strides; not on matrices
 *                       the plane-marching kernel takes): the rows are cut into tiles of 16, a tile is DESCRIBED by the union of its
 *                       columns in blocks of four plus a 64-bit occupancy mask per block (24 B per block instead of 4 B per entry;
 *                       the values stay where they are) when its rows ascend strictly, it holds 1..2048 entries and at least
 *                       "mv5_min_fill_pct" (default 25) percent of its 16 x 4 operand slots hold an entry; the other tiles' rows go to a
 *                       gather kernel.  1 (default) = use it when at most "mv5_max_other_pct" (default 50) percent of the rows are
 *                       left to the gather rows, 2 = whenever a tile can be described (no fill threshold: tests), 0 = never
 *     "mv_order"        row-block order: 2 (default) strips from the far stride found in the matrix (falls back to "mv_remap"),
 *                       1 XCD-contiguous (LDS-staged kernel), 0 "mv_remap": 0 dispatch, 1 XCD-contiguous, 2^k grouped (default 16)
 *     "mv_strip_min_kb" / "mv_strip_l2_kb"  when strips engage / how much of an XCD's L2 a strip's X rows may take
 *     "mv_glds"         LDS-staged kernel: X window through global_load_lds (1) or registers (0)
 *     "mv4_2d"          plane-marching kernel on 2-D lattices (lines grouped 32..128 at a time into the planes it marches through;
 *                       the first and last line of a group go to its gather rows): 1 (default) on, 0 off
 *     "mv4_xcol"        plane-marching kernel, column-major X (LayoutLeft): 1 (default) the X pieces of a plane are fetched column-wise
 *                       (whole cache lines per load) into slab rows swizzled in LDS; 0 the order used for general strides
 *     "mv4_wg_per_cu"   plane-marching kernel: workgroups per CU the split along the far stride aims for (default 8, 1..64)
 *     "march"           rank 1 on the plane-marching analysis (fp64 vectors, matrices that verify as lattice stencils): 0 (default)
 *                       off -- measured equal to the planned stream kernel on C2 --, 1 on; "march_planes" planes per workgroup (20)
 *   kkamd_spmv_struct (global only): "struct_remap", "struct_group", "struct_strip" workgroup orders, all off
 *   "verbose" (global): 1 = the library reports what it chose on stdout
 *   "mis2_lanes_per_vertex" (kkamd_set_default only): lanes per work-list vertex of the MIS-2 unit, 0 (default: from the mean degree) or
 *          a power of two up to 64; see kkamd_graph_d2_mis.  No output depends on it
 *   SpGEMM (kkamd_set_default only) "spgemm_win_bits" (columns per LDS bitmap pass), "spgemm_emit_win_bits" (the same for the rows that
 *          walk their products again in the numeric phase; 0 = spgemm_win_bits), "spgemm_val_cap" (entries of C per value window),
 *          "spgemm_force_unsorted", "spgemm_emit_chunked" (test hooks for alternative code paths);
 *          "spgemm_val_small_cnt", "spgemm_val_tiny_cnt" (rows of C with at most this many entries take the flat value kernel's 256- / 128-
 *          work-item shape; 0 = none), "spgemm_block" (1: rows of C that fill "spgemm_block_min_pct" % of the columns -- or
 *          "spgemm_block_la_pct" % with more than 512 entries in the A row -- take the column-block value kernels; 0: windows only),
 *          "spgemm_block_w" (columns per block, a power of two up to 16384), "spgemm_items" (1: those rows as items of up to
 *          "spgemm_item_blocks" blocks and "spgemm_item_cap" entries; 0: one workgroup per row and block),
 *          "spgemm_keep_bitmaps", "spgemm_keep_lists" (1: the symbolic phase keeps bitmaps / entry lists of its dense rows for the first
 *          numeric call; 0: those rows walk their products twice), "spgemm_pool_keep" (the process-wide store behind them when the last
 *          handle goes: 0 returned after the process's first product and kept for repeat users, 1 kept, 2 returned),
 *          "spgemm_emit_sort" (1: entries(C) of rows with more than 256 entries out of at most 2048 products are sorted in LDS, eight rows
 *          per CU; 0: they take the bitmap kernel like every other dense row), "spgemm_sym_units" (1, default: the symbolic phase counts its dense class
 *          by units = (row of C, window of columns), each a workgroup of its own around a 32 KB LDS bitmap, described by heads built from an
 *          index of B and of A's entries at window granularity; 0: one workgroup per row, as before round 6), "spgemm_unit_bits" (log2 of a
 *          unit's window, 6..18, default 18; small values are for tests), "spgemm_store_cap_mb" (upper limit, in MB, of the structure the
 *          symbolic phase keeps for the first numeric call; 0 = default: 0.225 of the free HBM; room goes to the heaviest rows first and
 *          rows past the limit walk their products again in the numeric phase), "spgemm_quad_rows" (wave-per-row kernels with four rows per wave, 16 lanes each: 1 = for the rows
 *          with at most 64 products (symbolic) / 32 entries (numeric) -- stencil and multigrid products --, 2 = for every row of the wave bin, 0 = never).
 * Knobs that switch parts of kernels OFF ("ablate", "lds_pad_kb", "struct_lds_pad_kb", "spgemm_debug") exist only in the
 * measurement build libkkamd_ablate.so (csrc: make ablate, -DKK_ABLATE); libkkamd.so answers KKAMD_ERR_INVALID_ARG. */
int kkamd_spmv_plan_set(kkamd_spmv_plan_t* plan, const char* key, int value);
int kkamd_set_default(const char* key, int value);
/* The caller has written to A.values since the plan's last SpMV.  The native CRS kernels read A.values at every call and need no
 * notice; a plan that keeps a RE-ORDERED COPY of the values (the cached transpose of modes T / H; the opt-in column-slab copy) copies
 * them again at its next call.  Under "values_tracking" 0 (default) and 2 the plan notices changes itself and this call is optional;
 * under 1 it is the only way the copies learn of a change.  No reference counterpart: the reference's handle holds no values
 * (sparse/src/KokkosSparse_spmv_handle.hpp:273-277), vendor analyses of this kind ask for the same call (rocsparse update-values). */
int kkamd_spmv_plan_values_changed(kkamd_spmv_plan_t* plan);
/* What the analysis of a plan produced: "tile" (nnz per workgroup, 0 = no tiling), "tiles", per-mode tile counts "plain_tiles" /
 * "code_tiles" / "staged_tiles" / "pattern_tiles", "pattern_list_identity" (1 if the pattern tiles are tiles 0 ... pattern_tiles - 1, so
 * that their launch reads no tile list), "window_codes" (1 if any tile uses the column analysis), "window_staged_x",
 * "plan_bytes" (HBM the analysis keeps), "transpose_cached", rank 2: "mv_tiles", "mv_staged_tiles", "mv_order" (order in use),
 * "mv_period" (far stride found), "mv_plan_bytes", plane-marching kernel: "mv4_workgroups" (0 = not in use), "mv4_other_rows"
 * (rows left to its gather kernel), "mv4_stencil" (entries of the stencil), "mv4_near_stride"; matrix-core kernel: "mv5_tiles" (described
 * 16-row tiles, 0 = not in use), "mv5_other_rows", "mv5_blocks" (column blocks = MFMA instructions per pass), "mv5_fill_permille"; nonzero-split kernel: "mv6_chunks" (0 = not in use),
 * "mv6_empty_rows"; "mv_long_rows" / "mv_long_nnz" (rows above the long-row threshold and their entries); "march_workgroups" (rank-1 marching kernel, 0 = not in use);
 * column-slab copy: "colslab" (1 = in use), "colslab_tried", "colslab_slabs", "colslab_shift", "colslab_bytes", and what the selection
 * measured, "colslab_crs_us" / "colslab_us" (microseconds per call of the CRS kernel / of the copy; 0 = not measured). */
int kkamd_spmv_plan_query(const kkamd_spmv_plan_t* plan, const char* key, int64_t* value);
/* Copies a per-tile array of the analysis to a HOST buffer of `count` int32: "tile_first_row" (tiles + 1 entries: the first row that
 * starts at or after nonzero b * tile, bit 31 set when the tile starts inside a row -- the nnz-split counterpart of the
 * reference's merge-path diagonal search, sparse/impl/KokkosSparse_merge_matrix.hpp:196-227) or "tile_mode" (tiles entries,
 * low two bits 0 plain / 1 codes / 2 codes + staged x / 3 row-pattern record). */
int kkamd_spmv_plan_export(const kkamd_spmv_plan_t* plan, const char* what, void* h_out, int64_t count);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU SpMV: the CrsMatrix is 1-D row-partitioned over the GPUs of one node, one process per GPU.  Rank r owns the row slab
 * [row_offsets[r], row_offsets[r+1]) of A (LOCAL row_map, GLOBAL column indices), the matching slab of y and shard of x; one
 * exchange of x entries per SpMV (RCCL over xGMI), no other communication.  The reference has no counterpart (upstream this is
 * Tpetra's job); the local SpMV is kkamd_spmv.
 *   exchange  0 auto (the column-range halo when it moves less than half of the all-gather, else the column-set halo when that
 *             does, else the all-gather), 1 halo by column RANGE (the x ranges the slab's columns span, contiguous pieces point to
 *             point straight into x), 2 all-gather (every shard to every rank through the transport's collective), 3 all-gather
 *             by peer-to-peer pulls (every rank maps the others' x buffers through hipIpc once and pulls world - 1 shards with
 *             concurrent copies between two 8-byte barrier collectives: all 7 xGMI links at once, no ring), 4 halo by column SET
 *             (the general importer: exactly the x entries the slab's off-slab columns name -- per-peer index lists agreed once,
 *             a pack kernel, point-to-point pieces, a scatter kernel), 5 all-gather in the form the operator picks BY TIMING at
 *             creation: every form the transport and the runtime offer (the collective; every shard to every peer point to point;
 *             peer-to-peer pulls) runs one warm-up and two timed exchanges with all ranks in step, and the form with the smallest
 *             maximum over the ranks stays.  Since round 6 the auto rule's all-gather is 5; 2 and 3 remain as forced forms;
 *   overlap   1: rows that reference only the rank's own x entries are computed while the halo is in flight.
 * Transport: by default RCCL, bound at run time from the librccl.so.1 already in the process; rank 0 obtains the 128-byte id
 * with kkamd_dist_unique_id and the host's launcher (MPI, torch.distributed, a file) hands it to every rank.  A host that
 * communicates otherwise passes its own kkamd_transport_t (both functions are stream-ordered; sizes in bytes).
 * ------------------------------------------------------------------------------------------------ */
typedef struct kkamd_dist_spmv kkamd_dist_spmv_t;
typedef struct {
  void* ctx;
  /* every rank contributes bytes_per_rank bytes; d_recv receives world * bytes_per_rank bytes in rank order */
  int (*all_gather)(void* ctx, const void* d_send, void* d_recv, int64_t bytes_per_rank, kkamd_stream_t stream);
  /* one batch of point-to-point transfers: nsend sends and nrecv receives, matched by peer */
  int (*exchange)(void* ctx, int nsend, const void* const* d_send, const int64_t* send_bytes, const int* send_peer, int nrecv,
                  void* const* d_recv, const int64_t* recv_bytes, const int* recv_peer, kkamd_stream_t stream);
} kkamd_transport_t;

int kkamd_dist_unique_id(void* id128);
/* Preflight of the built-in RCCL transport on the calling rank alone (no counterpart in the reference, which has no distributed
 * layer: cmake/fake_tribits.cmake:210 runs every test with NUM_MPI_PROCS 1): binds librccl, forms a ONE-rank communicator and runs
 * every entry point the N-rank exchanges use -- ncclAllGather in place and out of place, a group of ncclSend / ncclRecv to itself,
 * an empty group -- on `bytes` of device data that are compared afterwards.  A binding or ABI problem shows as an error code here
 * instead of a hang in the first exchange of an N-rank job. */
int kkamd_dist_transport_selftest(int64_t bytes, kkamd_stream_t stream);
/* world == 1 with id128 given and exchange != 0: the one-rank job still forms its RCCL communicator and runs the forced exchange
 * through it (the in-place ncclAllGather of one shard; groups with no peers) -- the N-rank code path on one GPU. */
int kkamd_dist_spmv_create(kkamd_dist_spmv_t** op, const kkamd_crs_t* A_local, const int64_t* row_offsets /* host, world + 1 */,
                           int world, int rank, const void* id128 /* NULL with a transport; optional when world == 1 */,
                           const kkamd_transport_t* transport /* NULL = RCCL */, int algorithm, int exchange, int overlap,
                           int vector_type, kkamd_stream_t stream);
int kkamd_dist_spmv_destroy(kkamd_dist_spmv_t* op);
/* x lives in a full-length buffer owned by the operator: *d_x_local is the rank's own window of it (a caller that keeps its x
 * shard there never copies it), *d_x_full the whole buffer.  Either pointer argument may be NULL. */
int kkamd_dist_spmv_x_local(kkamd_dist_spmv_t* op, void** d_x_local, void** d_x_full);
/* y_shard := alpha * A_local * exchanged(x) + beta * y_shard.  d_x_shard may be the pointer of kkamd_dist_spmv_x_local (no copy)
 * or any device buffer of the shard's length (copied in).  what: 0 the whole step, 1 the exchange only, 2 the local SpMV only
 * (measurement aids: 1 and 2 split a step into its two costs). */
int kkamd_dist_spmv_apply(kkamd_dist_spmv_t* op, double alpha, const void* d_x_shard, double beta, void* d_y_shard, int what,
                          kkamd_stream_t stream);
/* "exchange" (0 local, 1 halo by column range, 2 all-gather, 3 all-gather by peer-to-peer pulls, 4 halo by column set, 5 all-gather in
 * the timed form: "allgather_selected" 1, "allgather_form" 0 collective / 1 send-receive / 2 peer-to-peer pulls,
 * "allgather_us_collective" / "_sendrecv" / "_p2p" the maximum over the ranks measured at creation, -1 = form not offered), "exchange_bytes"
 * (received per SpMV), "interior_rows", "parts", "sends", "recvs", "part0_rows" (rows of the interior view, or of the slab when it is
 * not split) and "part0_<key>" = kkamd_spmv_plan_query(<key>) of that view's plan (e.g. "part0_pattern_tiles") */
int kkamd_dist_spmv_query(const kkamd_dist_spmv_t* op, const char* key, int64_t* value);

/* ------------------------------------------------------------------------------------------------
 * SpGEMM.  Replaces Impl::SPGEMM_SYMBOLIC<...>::spgemm_symbolic and
 * Impl::SPGEMM_NUMERIC<...>::spgemm_numeric (sparse/impl/KokkosSparse_spgemm_symbolic_spec.hpp:72-126,
 * ..._numeric_spec.hpp:91-145; vendor precedent sparse/tpls/KokkosSparse_spgemm_symbolic_tpl_spec_decl.hpp:367-,
 * ..._numeric_tpl_spec_decl.hpp:259-).  A is m x n, B is n x k, C is m x k.
 *
 * The handle is the analogue of SPGEMMHandle's cross-phase state (c_nnz, row flops, max nnz per row:
 * sparse/src/KokkosSparse_spgemm_handle.hpp:231-247).  Contract honoured: symbolic fills row_map C and
 * returns nnz(C); the caller allocates entries/values of that size; numeric fills both, with every row's
 * columns in ascending order (the reference sorts after numeric:
 * sparse/impl/KokkosSparse_spgemm_numeric_spec.hpp:138-140); numeric may be repeated with new values.
 * Inputs need not be sorted or merged.
 * ------------------------------------------------------------------------------------------------ */
typedef struct kkamd_spgemm_handle kkamd_spgemm_handle_t;

int kkamd_spgemm_create(kkamd_spgemm_handle_t** handle);
int kkamd_spgemm_destroy(kkamd_spgemm_handle_t* handle);

int kkamd_spgemm_symbolic(kkamd_spgemm_handle_t* handle, int64_t m, int64_t n, int64_t k, const void* d_row_mapA,
                          const int32_t* d_entriesA, const void* d_row_mapB, const int32_t* d_entriesB,
                          void* d_row_mapC, int offset_type, int64_t* c_nnz, kkamd_stream_t stream);

int kkamd_spgemm_numeric(kkamd_spgemm_handle_t* handle, int64_t m, int64_t n, int64_t k, const void* d_row_mapA,
                         const int32_t* d_entriesA, const void* d_valuesA, const void* d_row_mapB,
                         const int32_t* d_entriesB, const void* d_valuesB, const void* d_row_mapC,
                         int32_t* d_entriesC, void* d_valuesC, int offset_type, int value_type,
                         kkamd_stream_t stream);

/* Jacobi-fused product, KokkosSparse::Experimental::spgemm_jacobi (sparse/src/KokkosSparse_spgemm_jacobi.hpp:26-188; semantics
 * sparse/impl/KokkosSparse_spgemm_jacobi_seq_impl.hpp:65-123; what MueLu's SaPFactory reaches through Tpetra::MatrixMatrix::Jacobi):
 *     C = (I - omega D^-1 A) B = B - omega D^-1 (A B),    A square (m == n), d_dinv = the m values 1 / a_ii, of the value type.
 * Called in the place of kkamd_spgemm_numeric: kkamd_spgemm_symbolic(A, B) has completed on the handle, row_mapC is its output, entriesC and
 * valuesC have c_nnz entries; rows of C leave column-sorted; the call may be repeated with new values, omega or dinv, and entries(C) are
 * kept across calls as kkamd_spgemm_numeric keeps them ("entries_computed").  Statuses: those of kkamd_spgemm_numeric (KKAMD_ERR_STATE before
 * the symbolic phase or with other dimensions, KKAMD_ERR_UNSUPPORTED for another value type); m != n, or a null d_dinv with c_nnz > 0:
 * KKAMD_ERR_INVALID_ARG.
 *
 * Values.  With VT the value type and fl() one rounding to VT:
 *     w      = VT(omega)
 *     mult_i = fl(-w * dinv_i)
 *     a'_ij  = fl(a_ij * mult_i)                                   for every stored entry of A (a buffer of nnz(A) values the handle owns)
 *     N      = what kkamd_spgemm_numeric computes for (A', B) on this handle: the same kernels on the same bins (bit for bit the same
 *              wherever one wave owns a row's accumulator; where several waves add into one with floating-point atomics, in the order
 *              they arrive, as two calls of kkamd_spgemm_numeric differ from each other)
 *     c_ik   = fl(N_ik + b_ik)                                     for every stored entry (i, k) of row i of B; a column stored several times
 *                                                                  in the row is added once per copy, one after another in stored order
 *     c_ik   = N_ik                                                everywhere else
 * The reference's sequential form puts b_ik into the accumulator first and the products after it (its parallel forms define no order);
 * here it joins last.  omega == 0 takes no shortcut (a'_ij = -0 * ..., signed zeros and NaN as the arithmetic gives them); Inf and NaN in
 * A, B or dinv propagate as these five lines say.
 *
 * Pattern.  Every column of row i of B must occur in row i of C = pattern(A B).  It does whenever every row of A stores its diagonal.  The
 * reference assumes it and writes past the row of C otherwise; here the call returns KKAMD_ERR_INVALID_ARG, the message naming the smallest
 * such row, and values(C) are unspecified.
 *
 * Three steps on the stream, one synchronisation: a kernel writes a'; the numeric phase runs on (row_mapA, entriesA, a'); a kernel adds the
 * rows of B, finding every column in its ascending row of C by bisection, without floating-point atomics.  When every row of B is strictly
 * ascending (checked on the device in every call) a group of lanes shares a row -- about four entries of B's mean row per lane, 1..64 lanes --
 * otherwise one lane walks each row in stored order.  kkamd_spgemm_get 24 / 25 and a "verbose" line say which. */
int kkamd_spgemm_jacobi(kkamd_spgemm_handle_t* handle, int64_t m, int64_t n, int64_t k, const void* d_row_mapA,
                        const int32_t* d_entriesA, const void* d_valuesA, const void* d_row_mapB,
                        const int32_t* d_entriesB, const void* d_valuesB, const void* d_row_mapC,
                        int32_t* d_entriesC, void* d_valuesC, double omega, const void* d_dinv /* m values of value_type */,
                        int offset_type, int value_type, kkamd_stream_t stream);

/* Options: what SPGEMMHandle / KokkosKernelsHandle setters map to (sparse/src/KokkosSparse_spgemm_handle.hpp:427-501,562-616;
 * sparse/src/KokkosKernels_Handle.hpp:380-465).  Set before the phase they shape.
 *   "algorithm"            SPGEMMAlgorithm value: SPGEMM_KK (default) and its aliases KK_MEMORY / KK_SPEED / KK_MEMSPEED / KK_LP run the
 *                          LDS hash-accumulator numeric; SPGEMM_KK_DENSE runs the dense-accumulator numeric (impl_speed.hpp:28-150);
 *                          SPGEMM_DEBUG / SPGEMM_SERIAL (host-sequential in the reference; every algorithm's C leaves the public
 *                          spgemm_numeric sorted, numeric_spec.hpp:138-140, so their C is everybody's C) run the hash algorithm
 *   "accumulator"          SPGEMMAccumulator: 1 = dense (same as SPGEMM_KK_DENSE), 0 / 2 = hash
 *   "compression"          B compression for the symbolic phase (impl_compression.hpp): 0 off (default), 1 keep when it pays, 2 always
 *   "compression_cut_off"  keep the compressed B when it leaves at most this share of the symbolic work (default 0.85)
 *   "verbose"              1: chosen algorithm, row bins, kernels and compression decision on stdout (KOKKOSKERNELS_VERBOSE)
 *   "entries_computed"     the reference's are_entries_computed() as the caller knows it: 0 forces the next numeric call to write
 *                          entries(C) again (re-allocated / overwritten arrays); 1 leaves the decision to the handle, which keeps
 *                          entries(C) across numeric calls only when it wrote them into the same row_map / entries arrays itself
 *                          (numeric reuse, sparse/tpls/KokkosSparse_spgemm_numeric_tpl_spec_decl.hpp:288-329)
 *   "symbolic_computed"    0: the handle forgets its symbolic phase, so that the next kkamd_spgemm_symbolic analyses again even when it is
 *                          given the same row map arrays (it otherwise answers a repeated call on the same arrays from memory, as the
 *                          reference does): for a caller that rewrote those arrays in place with another pattern; 1 changes nothing
 * Hints -- accepted, recorded, reported under "verbose", without effect, exactly as the reference's rocSPARSE / cuSPARSE paths treat
 * them (the reference's driver and unit tests set them before every spgemm: perf_test/sparse/KokkosSparse_spgemm.cpp:311-317,378-399,
 * sparse/unit_test/Test_Sparse_spgemm.hpp:91-92): "team_work_size", "shmem_size", "suggested_team_size", "suggested_vector_size",
 * "dynamic_scheduling", "min_hash_size_scale", "first_level_hash_cut_off", "mkl_sort_option", "mkl_keep_output",
 * "mkl_convert_to_1base", "multi_color_scale", "read_write_cost_calc", "compression_steps", "max_col_dense_acc", "sort_option"
 * (rows of C always leave column-sorted).  Any other key: KKAMD_ERR_INVALID_ARG. */
int kkamd_spgemm_set(kkamd_spgemm_handle_t* handle, const char* key, double value);
/* what: 0 c_nnz, 1 total multiplications (the reference's original_overall_flops / 2),
 * 2 max row flops, 3 max nnz in a row of C, 4 symbolic called, 5 numeric called, 6 B was compressed for the symbolic phase,
 * 7 symbolic insertions after compression, 8 numeric algorithm in use (0 hash, 1 dense accumulator), 9 the SPGEMMAlgorithm value the
 * caller set (4 = SPGEMM_DEFAULT until then), 10 number of distinct hints recorded, 11 the last numeric call kept the entries(C)
 * of the dense rows from the previous call (numeric reuse), 12 rows whose entries(C) the last numeric call wrote from a bitmap kept by the
 * symbolic phase, 13 bitmaps the symbolic phase holds at this moment (they are freed by the numeric call that uses them), 14 rows whose entries(C) the
 * last numeric call copied from the entry lists the symbolic phase left (dense rows whose bitmap is not kept), 15 rows whose entries(C)
 * the last numeric call sorted in LDS (rows of more than 256 entries out of at most 2048 products), 16 - 18 rows / items of the column-block
 * value kernel, 19 units (row of C, window of 2^18 columns) the last symbolic phase counted its dense class by (0: none, or row by row),
 * 20 units whose bitmap it kept for the numeric phase, 21 rows of the class whose every unit kept its structure (bitmap or entry list),
 * 22 bytes the process-wide store of kept structure holds at this moment, 23 the most it has held (process-wide; both are independent of
 * the handle passed; kkamd_release_scratch returns the store to the device), 24 lanes per row of B in the last kkamd_spgemm_jacobi call's
 * epilogue, 25 that epilogue took the fast form (1: every row of B strictly ascending; 0: one lane per row, stored order).
 * With units, 12 counts the rows whose entries(C) the last numeric call wrote from kept units, 13 the rows held, 14 those of 12 with at
 * least one unit kept as an entry list. */
int kkamd_spgemm_get(kkamd_spgemm_handle_t* handle, int what, int64_t* value);
/* the recorded value of a hint key (the reference's get_* of the same setter); KKAMD_ERR_INVALID_ARG when the key was never set */
int kkamd_spgemm_get_hint(kkamd_spgemm_handle_t* handle, const char* key, double* value);

/* Row-partitioned SpGEMM over the GPUs of one node: rank r owns the row slab [row_offsets[r], row_offsets[r+1]) of A (LOCAL row_map)
 * and of C = A*B; B is replicated on every GPU, so there is no data-path communication at all (this is what lets BASELINE config 4
 * as specified -- R-MAT scale 22, nnz(C) = 7.2e10 = 863 GB -- fit eight GPUs).  No reference counterpart (upstream: Tpetra).
 *   _partition  contiguous slabs of near-equal MULTIPLICATIONS (row flops of sparse/impl/KokkosSparse_spgemm_impl_symbolic.hpp:1108-1185,
 *               computed on the device from the full A and B structure): fills row_offsets[world + 1] (host) and, when given,
 *               the multiplications of every slab; every rank that calls it with the same A and B gets the same answer.
 *   _symbolic / _numeric / _jacobi   kkamd_spgemm_symbolic / _numeric / _jacobi on the rank's slab (checked against the partition), state in the operator;
 *   _handle     the operator's SpGEMM handle, for kkamd_spgemm_set / _get;
 *   _query      "row0", "rows_local", "rows_global", "c_nnz_local", "mults_local". */
typedef struct kkamd_dist_spgemm kkamd_dist_spgemm_t;
int kkamd_dist_spgemm_partition(int64_t m, const void* d_row_mapA, const int32_t* d_entriesA, const void* d_row_mapB, int offset_type, int world,
                                int64_t* row_offsets /* host, world + 1 */, int64_t* mults_per_rank /* host, world, or NULL */, kkamd_stream_t stream);
int kkamd_dist_spgemm_create(kkamd_dist_spgemm_t** op, int world, int rank, const int64_t* row_offsets /* host, world + 1 */);
int kkamd_dist_spgemm_destroy(kkamd_dist_spgemm_t* op);
kkamd_spgemm_handle_t* kkamd_dist_spgemm_handle(kkamd_dist_spgemm_t* op);
int kkamd_dist_spgemm_symbolic(kkamd_dist_spgemm_t* op, int64_t m_local, int64_t n, int64_t k, const void* d_row_mapA_local, const int32_t* d_entriesA_local,
                               const void* d_row_mapB, const int32_t* d_entriesB, void* d_row_mapC_local, int offset_type, int64_t* c_nnz_local,
                               kkamd_stream_t stream);
int kkamd_dist_spgemm_numeric(kkamd_dist_spgemm_t* op, int64_t m_local, int64_t n, int64_t k, const void* d_row_mapA_local, const int32_t* d_entriesA_local,
                              const void* d_valuesA_local, const void* d_row_mapB, const int32_t* d_entriesB, const void* d_valuesB,
                              const void* d_row_mapC_local, int32_t* d_entriesC_local, void* d_valuesC_local, int offset_type, int value_type,
                              kkamd_stream_t stream);
/* kkamd_spgemm_jacobi on the rank's slab: local row i of C adds global row row_offsets[rank] + i of the replicated B; d_dinv_local holds the
 * slab's m_local inverse diagonals.  The global matrix must be square (n == the partition's rows).  No communication. */
int kkamd_dist_spgemm_jacobi(kkamd_dist_spgemm_t* op, int64_t m_local, int64_t n, int64_t k, const void* d_row_mapA_local, const int32_t* d_entriesA_local,
                             const void* d_valuesA_local, const void* d_row_mapB, const int32_t* d_entriesB, const void* d_valuesB,
                             const void* d_row_mapC_local, int32_t* d_entriesC_local, void* d_valuesC_local, double omega, const void* d_dinv_local,
                             int offset_type, int value_type, kkamd_stream_t stream);
int kkamd_dist_spgemm_query(const kkamd_dist_spgemm_t* op, const char* key, int64_t* value);


/* ------------------------------------------------------------------------------------------------
 * Sparse triangular solve.  Replaces KokkosSparse::sptrsv_symbolic / sptrsv_solve for a CrsMatrix triangle
 * (sparse/src/KokkosSparse_sptrsv.hpp:54-122,268-411; native level scheduling sparse/impl/KokkosSparse_sptrsv_symbolic_impl.hpp:156-214
 * and :569-640, solve semantics sparse/impl/KokkosSparse_sptrsv_solve_impl.hpp:434-566; the reference's only vendor plug-in is cuSPARSE,
 * sparse/tpls/KokkosSparse_sptrsv_*_tpl_spec_*.hpp).  Solves L x = b or U x = b for a square CRS triangle whose diagonal is stored:
 * x[i] = (b[i] - sum_{j != i} a_ij x[j]) / a_ii.  Entries of a row may come in any order, repeated off-diagonal columns are summed, b may
 * be x, the old content of x is never read.  b and x are rank 1 and contiguous (the reference static-asserts rank 1, :291-292); type pairs
 * (F64,F64) and (F32,F32).
 *
 * The handle is the analogue of SPTRSVHandle (sparse/src/KokkosSparse_sptrsv_handle.hpp): it keeps the level sets -- level_list,
 * nodes_per_level, nodes_grouped_by_level, defined exactly as in the reference: level(i) = 1 + max level(col) over the row's off-diagonal
 * columns, 1 for a row without any; rows ascending inside a level -- and every row's diagonal position, never values.
 * ------------------------------------------------------------------------------------------------ */
typedef struct kkamd_sptrsv_handle kkamd_sptrsv_handle_t;
/* KokkosSparse::Experimental::SPTRSVAlgorithm (sparse/src/KokkosSparse_sptrsv_handle.hpp:42-47).  The three level-scheduled values run
 * the same kernels, one launch per level: RP with one lane per row and no chaining, TP1 with the lanes per row chosen per level (the smallest power of two
 * that covers the level's mean row length), TP1CHAIN the same plus runs of narrow levels chained into single-workgroup launches (the reference's TP1CHAIN
 * idea).  SPTRSV_CUSPARSE returns KKAMD_ERR_UNSUPPORTED at create. */
typedef enum {
  KKAMD_SPTRSV_SEQLVLSCHD_RP       = 0,
  KKAMD_SPTRSV_SEQLVLSCHD_TP1      = 1,
  KKAMD_SPTRSV_SEQLVLSCHD_TP1CHAIN = 2,
  KKAMD_SPTRSV_CUSPARSE            = 3
} kkamd_sptrsv_algorithm;
/* KokkosKernelsHandle::create_sptrsv_handle(algm, nrows, lower_tri) / destroy_sptrsv_handle (sparse/src/KokkosKernels_Handle.hpp:777-797) */
int kkamd_sptrsv_create(kkamd_sptrsv_handle_t** handle, int algorithm, int64_t num_rows, int lower_tri);
int kkamd_sptrsv_destroy(kkamd_sptrsv_handle_t* handle);
/* sptrsv_symbolic(handle, rowmap, entries) (sparse/src/KokkosSparse_sptrsv.hpp:54-122).  Validates first, in one pass that indexes nothing
 * by a column it has not yet checked -- KKAMD_ERR_INVALID_ARG, the first offending row named in kkamd_last_error(), when num_rows differs
 * from the handle's, a column is outside [0, num_rows), an entry is on the wrong side of the diagonal, or a row has no or more than one
 * diagonal entry --, then builds the level sets on the device (no host pass over the entries; one stream synchronisation per level).  May be
 * repeated on one handle (analyses again).  Synchronises the stream, because it returns counts. */
int kkamd_sptrsv_symbolic(kkamd_sptrsv_handle_t* handle, int64_t num_rows, const void* d_row_map, const int32_t* d_entries, int offset_type,
                          kkamd_stream_t stream);
/* sptrsv_solve(handle, rowmap, entries, values, b, x) (sparse/src/KokkosSparse_sptrsv.hpp:268-411).  KKAMD_ERR_STATE before a completed
 * symbolic call, KKAMD_ERR_UNSUPPORTED for another value type; otherwise asynchronous on the stream: allocates nothing, synchronises
 * nothing, reads the caller's arrays at every call (the structure must be the one analysed). */
int kkamd_sptrsv_solve(kkamd_sptrsv_handle_t* handle, int64_t num_rows, const void* d_row_map, const int32_t* d_entries, const void* d_values,
                       const void* d_b, void* d_x, int offset_type, int value_type, kkamd_stream_t stream);
/* Knobs (values outside the ranges: KKAMD_ERR_INVALID_ARG; the analogue of SPTRSVHandle::set_team_size / set_vector_size /
 * set_chain_threshold, sptrsv_handle.hpp:749-760,860-870):
 *   "lanes_per_row"  0 (default) = by level, or 1, 2, 4, ..., 64; ignored by SEQLVLSCHD_RP
 *   "chain_rows"     a level with at most this many rows may join a chain (SEQLVLSCHD_TP1CHAIN only); 0 = never; default 64 (measured:
 *                    DESIGN.md 4.5; the reference defaults its threshold to the team size)
 *   "chain_levels"   the most levels one chain launch covers (>= 1, default 1024): bounds how long a single launch runs */
int kkamd_sptrsv_set(kkamd_sptrsv_handle_t* handle, const char* key, int value);
/* "num_levels", "symbolic_complete", "lower_tri", "algorithm", "num_rows", "max_level_rows", "launches" (kernel launches of one solve),
 * "chain_launches", "chained_levels", "plan_bytes" (HBM the handle keeps), and the three knobs */
int kkamd_sptrsv_get(const kkamd_sptrsv_handle_t* handle, const char* key, int64_t* value);
/* to a HOST buffer of `count` int32: "level_list" (num_rows entries, 1-based levels as in the reference), "nodes_per_level" (num_levels),
 * "nodes_grouped_by_level" (num_rows) */
int kkamd_sptrsv_export(const kkamd_sptrsv_handle_t* handle, const char* what, void* h_out, int64_t count);

/* ------------------------------------------------------------------------------------------------
 * Incomplete LU factorisation with level of fill k, ILU(k).  Replaces KokkosSparse::spiluk_symbolic / spiluk_numeric for a square
 * CrsMatrix (sparse/src/KokkosSparse_spiluk.hpp:42-197,200-415; handle sparse/src/KokkosSparse_spiluk_handle.hpp:31-247; native
 * symbolic loop sparse/impl/KokkosSparse_spiluk_symbolic_impl.hpp:212-418, numeric functor sparse/impl/KokkosSparse_spiluk_numeric_impl.hpp:438-551,
 * level loop :572-617).  The factors are what kkamd_sptrsv_* takes: row i of L holds the columns < i and then the unit diagonal, row i of
 * U the diagonal (present even when A has none) and then the columns > i, both sorted by column.  int32 ordinals, int32 or int64 offsets
 * (one type for A, L and U), values F64 or F32.
 *
 * The handle is the analogue of SPILUKHandle: nnzL, nnzU, the level sets of L (level_list, level_ptr, level_idx as the reference's handle
 * holds them) and this library's knobs, never values.  Not implemented: the block (BSR) variant, spiluk_numeric_streams, a device-side
 * fill computation, the reference-side TPL binding.
 * ------------------------------------------------------------------------------------------------ */
typedef struct kkamd_spiluk_handle kkamd_spiluk_handle_t;
/* KokkosSparse::Experimental::SPILUKAlgorithm (sparse/src/KokkosSparse_spiluk_handle.hpp:31-33): the reference has one */
typedef enum { KKAMD_SPILUK_SEQLVLSCHD_TP1 = 0 } kkamd_spiluk_algorithm;
/* KokkosKernelsHandle::create_spiluk_handle(algm, nrows, nnzL, nnzU) / destroy_spiluk_handle (sparse/src/KokkosKernels_Handle.hpp);
 * nnzL and nnzU are the caller's estimates, replaced by the true counts at symbolic (spiluk_handle.hpp:102-121,190-199) */
int kkamd_spiluk_create(kkamd_spiluk_handle_t** handle, int algorithm, int64_t num_rows, int64_t nnzL, int64_t nnzU);
int kkamd_spiluk_destroy(kkamd_spiluk_handle_t* handle);
/* spiluk_symbolic(handle, fill_lev, A_rowmap, A_entries, L_rowmap, L_entries, U_rowmap, U_entries) (sparse/src/KokkosSparse_spiluk.hpp:42-197;
 * sparse/impl/KokkosSparse_spiluk_symbolic_impl.hpp:212-418).  Writes the graphs of L and U for the sum-rule level of fill (entries of A
 * have level 0; eliminating row i by pivot j, pivots ascending, gives column c of U row j the level lev(i,j) + lev(j,c) + 1, kept when
 * <= fill_lev; an existing entry takes the minimum) and records nnzL, nnzU and the level sets of L.  L_capacity / U_capacity are the
 * extents of d_L_entries / d_U_entries: when one is too small nothing is written and KKAMD_ERR_INVALID_ARG comes back with the reference's
 * text "... must be larger than <capacity>, must be at least <nnz>" (:353-357,375-379) carrying the true count.  Checked before anything
 * is indexed (KKAMD_ERR_INVALID_ARG, first offending row named): num_rows equal to the handle's, A's row map ascending, columns in
 * [0, num_rows), no column twice in a row of A (the reference overwrites in a race there); fill_lev < 0 gives the reference's message
 * (spiluk.hpp:127-131).  The fill computation runs on the host, as in the reference; the level sets come from the device routine of
 * kkamd_sptrsv_symbolic.  May be repeated on one handle.  Synchronises the stream, because it returns counts. */
int kkamd_spiluk_symbolic(kkamd_spiluk_handle_t* handle, int fill_lev, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries,
                          void* d_L_row_map, int32_t* d_L_entries, int64_t L_capacity, void* d_U_row_map, int32_t* d_U_entries, int64_t U_capacity,
                          int offset_type, kkamd_stream_t stream);
/* spiluk_numeric(handle, fill_lev, A_rowmap, A_entries, A_values, L_rowmap, L_entries, L_values, U_rowmap, U_entries, U_values)
 * (sparse/src/KokkosSparse_spiluk.hpp:200-415; sparse/impl/KokkosSparse_spiluk_numeric_impl.hpp:438-551,572-617).  KKAMD_ERR_STATE before
 * a completed symbolic call, KKAMD_ERR_UNSUPPORTED for another value type; otherwise asynchronous on the stream: allocates nothing,
 * synchronises nothing, reads A at every call (new values on the analysed pattern need no second symbolic call).  The old content of
 * L_values / U_values is never read.  A zero pivot U(i,i) is replaced by 1e6 as in the reference (:528-534).  Deterministic: every entry
 * takes its updates one pivot at a time in ascending order, whatever the knobs. */
int kkamd_spiluk_numeric(kkamd_spiluk_handle_t* handle, int fill_lev, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries,
                         const void* d_A_values, const void* d_L_row_map, const int32_t* d_L_entries, void* d_L_values, const void* d_U_row_map,
                         const int32_t* d_U_entries, void* d_U_values, int offset_type, int value_type, kkamd_stream_t stream);
/* Knobs (values outside the ranges: KKAMD_ERR_INVALID_ARG; the analogue of SPILUKHandle::set_team_size / set_vector_size,
 * spiluk_handle.hpp:231-235), with the meaning and defaults of kkamd_sptrsv_set:
 *   "lanes_per_row"  0 (default) = the smallest power of two that covers the mean row of U, or 1, 2, 4, ..., 64
 *   "chain_rows"     a level with at most this many rows may join a chain; 0 = never; default 64
 *   "chain_levels"   the most levels one chain launch covers (>= 1, default 1024) */
int kkamd_spiluk_set(kkamd_spiluk_handle_t* handle, const char* key, int value);
/* "nnzL", "nnzU", "num_levels", "max_level_rows", "symbolic_complete", "algorithm", "num_rows", "launches" (kernel launches of one
 * numeric call), "chain_launches", "chained_levels", "plan_bytes" (HBM the handle keeps; at most 64 (num_rows + nnzL + nnzU) + 4096),
 * the three knobs, "lanes_in_use", "stage_entries_per_lane" (a row of up to this many entries per lane, L and U parts together, is staged
 * in LDS), "symbolic_fill_us" / "symbolic_other_us" (the host fill loop and the rest of the last symbolic call) */
int kkamd_spiluk_get(const kkamd_spiluk_handle_t* handle, const char* key, int64_t* value);
/* to a HOST buffer of `count` int32: "level_list" (num_rows entries, 1-based levels as in the reference), "level_ptr" (num_levels + 1),
 * "level_idx" (num_rows: the rows grouped by level) */
int kkamd_spiluk_export(const kkamd_spiluk_handle_t* handle, const char* what, void* h_out, int64_t count);

/* ------------------------------------------------------------------------------------------------
 * Point multicolor Gauss-Seidel.  Replaces KokkosSparse::gauss_seidel_symbolic / gauss_seidel_numeric / symmetric_gauss_seidel_apply /
 * forward_sweep_gauss_seidel_apply / backward_sweep_gauss_seidel_apply for a CrsMatrix (sparse/src/KokkosSparse_gauss_seidel.hpp; handle
 * sparse/src/KokkosSparse_gauss_seidel_handle.hpp; native implementation sparse/impl/KokkosSparse_gauss_seidel_impl.hpp: symbolic :697-830,
 * the row update :159-179, point_apply :1401-1466, the sweep order :1496-1560).  A has num_rows rows and num_cols >= num_rows columns; the
 * columns >= num_rows are ghost columns: read, never written, ignored by the colouring.  Every row stores its diagonal exactly once.
 * int32 ordinals, int32 or int64 offsets, values F64 or F32.
 *
 * The colouring is Jones-Plassmann on the device with the priority pair (h(i), i), where for the 32-bit unsigned x = i
 *     x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16;   h(i) = x      (arithmetic modulo 2^32)
 * and (h(j), j) > (h(i), i) when h(j) > h(i), or h(j) == h(i) and j > i.  It equals the sequential greedy colouring (smallest colour no
 * coloured neighbour holds) of the rows taken in descending priority: a function of the graph alone, the same on every run.
 *
 * The handle is the analogue of PointGaussSeidelHandle: colours, the permutation, the permuted matrix, the inverse diagonal, the permuted
 * work vectors, and this library's knobs.  Not implemented: block / BSR Gauss-Seidel (block_gauss_seidel_*), GS_CLUSTER, GS_TWOSTAGE, the
 * overloads that take execution-space instances (the _streams form of the handle), the reference-side TPL binding.
 * ------------------------------------------------------------------------------------------------ */
typedef struct kkamd_gs_handle kkamd_gs_handle_t;
/* KokkosSparse::GSAlgorithm (sparse/src/KokkosSparse_gauss_seidel_handle.hpp:30).  GS_DEFAULT, GS_PERMUTED and GS_TEAM run this
 * implementation (GS_PERMUTED: one lane per row unless "lanes_per_row" is set); GS_CLUSTER and GS_TWOSTAGE: KKAMD_ERR_UNSUPPORTED */
typedef enum {
  KKAMD_GS_DEFAULT  = 0,
  KKAMD_GS_PERMUTED = 1,
  KKAMD_GS_TEAM     = 2,
  KKAMD_GS_CLUSTER  = 3,
  KKAMD_GS_TWOSTAGE = 4
} kkamd_gs_algorithm;
/* KokkosSparse::GSDirection (gauss_seidel_handle.hpp:31) */
typedef enum { KKAMD_GS_FORWARD = 0, KKAMD_GS_BACKWARD = 1, KKAMD_GS_SYMMETRIC = 2 } kkamd_gs_direction;
/* KokkosKernelsHandle::create_gs_handle(GSAlgorithm) / destroy_gs_handle (sparse/src/KokkosKernels_Handle.hpp:581-628,715-720) */
int kkamd_gs_create(kkamd_gs_handle_t** handle, int algorithm);
int kkamd_gs_destroy(kkamd_gs_handle_t* handle);
/* gauss_seidel_symbolic(handle, num_rows, num_cols, row_map, entries, is_graph_symmetric) (sparse/src/KokkosSparse_gauss_seidel.hpp:45-134).
 * Validates first (KKAMD_ERR_INVALID_ARG naming the smallest offending row: row map not ascending, a column outside [0, num_cols), no
 * diagonal entry, more than one), colours the graph of the leading num_rows x num_rows block -- of A + A^T when is_graph_symmetric is 0 --
 * groups the rows by colour (ascending inside a colour, the rows with more than "long_row_threshold" entries at the end of their colour,
 * gauss_seidel_impl.hpp:787-810) and builds the permuted graph.  d_colors: NULL, or num_rows 1-based colours of the caller's (the reference
 * lets the caller choose the colouring algorithm; this is the place for a known colouring such as red-black).  They are checked in one pass:
 * a colour outside [1, num_rows] or two adjacent rows of one colour is KKAMD_ERR_INVALID_ARG naming the smallest offending row.
 * May be repeated on one handle; a failed call leaves the handle without an analysis.  Synchronises the stream. */
int kkamd_gs_symbolic(kkamd_gs_handle_t* handle, int64_t num_rows, int64_t num_cols, const void* d_row_map, const int32_t* d_entries,
                      int offset_type, int is_graph_symmetric, const int32_t* d_colors, kkamd_stream_t stream);
/* gauss_seidel_numeric(handle, num_rows, num_cols, row_map, entries, values[, given_inverse_diagonal], is_graph_symmetric)
 * (gauss_seidel.hpp:173-370): gathers the values into the permuted order and stores 1 / a_ii per row, or d_inverse_diagonal (num_rows
 * entries in the caller's row order; NULL = compute).  A zero diagonal gives Inf / NaN as in the reference.  KKAMD_ERR_STATE before a
 * completed symbolic call.  May be repeated with new values.  Asynchronous on the stream. */
int kkamd_gs_numeric(kkamd_gs_handle_t* handle, int64_t num_rows, int64_t num_cols, const void* d_row_map, const int32_t* d_entries,
                     const void* d_values, const void* d_inverse_diagonal, int offset_type, int value_type, kkamd_stream_t stream);
/* {symmetric,forward_sweep,backward_sweep}_gauss_seidel_apply(handle, num_rows, num_cols, row_map, entries, values, x, y, init_zero_x_vector,
 * update_y_vector, omega, numIter) (gauss_seidel.hpp:372-760).  x has num_cols rows, y num_rows rows, both num_vecs >= 1 columns; element
 * (i, v) is at d[i * row_stride + v * col_stride], so rank 1, LayoutLeft and LayoutRight are one entry point.  direction: a
 * kkamd_gs_direction; one symmetric iteration is a forward sweep (colours 1..C) and then a backward sweep (C..1).  Every row update is
 * x_i += omega * (y_i - sum_j a_ij x_j) * inv_diag_i with the diagonal term inside the sum (gauss_seidel_impl.hpp:159-179).
 * Runs the numeric phase itself when none has run since the last symbolic call (:1473).  update_y = 0 reuses the permuted y of the
 * previous apply: KKAMD_ERR_STATE when there is none or num_vecs changed.  init_zero_x != 0: x is not read, and all num_cols entries of x
 * are written (ghost entries become 0, as in the reference).  KKAMD_ERR_STATE before a symbolic call.  Deterministic: no floating-point
 * atomic, the same bits on every run and for every column whatever num_vecs is (columns go through the kernel in batches of 4). */
int kkamd_gs_apply(kkamd_gs_handle_t* handle, int64_t num_rows, int64_t num_cols, const void* d_row_map, const int32_t* d_entries,
                   const void* d_values, void* d_x, int64_t x_row_stride, int64_t x_col_stride, const void* d_y, int64_t y_row_stride,
                   int64_t y_col_stride, int64_t num_vecs, int init_zero_x, int update_y, double omega, int num_iter, int direction,
                   int offset_type, int value_type, kkamd_stream_t stream);
/* Knobs (values outside the ranges: KKAMD_ERR_INVALID_ARG), the first three with the meaning and defaults of kkamd_sptrsv_set, a colour in
 * the place of a level:
 *   "lanes_per_row"       0 (default) = the smallest power of two that covers a quarter of the launch's mean row (about four entries per
 *                         lane; measured), or 1, 2, 4, ..., 64
 *   "chain_rows"          a colour with at most this many rows may join a chain; 0 = never; default 64
 *   "chain_levels"        the most colours one chain launch covers (>= 1, default 1024)
 *   "long_row_threshold"  PointGaussSeidelHandle::set_long_row_threshold (gauss_seidel_handle.hpp:346): rows with more entries go to the end
 *                         of their colour and get one wave each; 0 (default) = none.  Read by the next symbolic call. */
int kkamd_gs_set(kkamd_gs_handle_t* handle, const char* key, int value);
/* "num_colors", "coloring_rounds" (0 for given colours), "num_rows", "num_cols", "symbolic_complete", "numeric_complete", "algorithm",
 * "long_rows", "long_row_threshold", "tail_launches" (long-row launches of one sweep, beyond "launches"), "num_levels" (= num_colors),
 * "max_level_rows", "launches" (colour and chain launches of one sweep), "chain_launches", "chained_levels", the three schedule knobs, and
 * "plan_bytes": HBM the handle keeps, at most 48 num_rows + 12 nnz + 8 num_vecs (num_rows + num_cols) + 16 */
int kkamd_gs_get(const kkamd_gs_handle_t* handle, const char* key, int64_t* value);
/* to a HOST buffer of `count` int32: "colors" (num_rows entries, 1-based, original row order), "color_xadj" (num_colors + 1),
 * "color_adj" (num_rows: the rows grouped by colour, which is the permutation new -> old), "old_to_new" (num_rows) */
int kkamd_gs_export(const kkamd_gs_handle_t* handle, const char* what, void* h_out, int64_t count);

/* ------------------------------------------------------------------------------------------------
 * Preconditioners.  Replaces KokkosSparse::Experimental::Preconditioner<CRS> and its two implementations
 * (sparse/src/KokkosSparse_Preconditioner.hpp:55-112, KokkosSparse_MatrixPrec.hpp:45-101, KokkosSparse_LUPrec.hpp:43-119).
 * apply: y := alpha * M x + beta * y on n-vectors of the matrix's value type; beta == 0 does not read y.  The matrices' arrays are
 * borrowed for the life of the preconditioner, as the reference's classes hold views.
 * ------------------------------------------------------------------------------------------------ */
typedef struct kkamd_precond kkamd_precond_t;
/* what the C++ virtual Preconditioner::apply binds to, and how a Gauss-Seidel or any foreign preconditioner comes in */
typedef int (*kkamd_precond_fn)(void* ctx, const void* d_x, void* d_y, double alpha, double beta, int value_type, kkamd_stream_t stream);
/* MatrixPrec(mat) (KokkosSparse_MatrixPrec.hpp:57-83): apply is spmv("N", alpha, M, x, beta, y) through a plan of its own */
int kkamd_precond_create_matrix(kkamd_precond_t** p, const kkamd_crs_t* M, kkamd_stream_t stream);
/* LUPrec(L, U) (KokkosSparse_LUPrec.hpp:64-101): y := alpha * U^-1 L^-1 x + beta * y with two kkamd_sptrsv handles (SEQLVLSCHD_TP1) that
 * are analysed ONCE, here; the reference calls sptrsv_symbolic again at every apply (:94-98).  L with its (unit) diagonal stored, U with its
 * diagonal stored, as kkamd_spiluk_numeric leaves them.  "LUPrec: L.numRows() != U.numRows()" is KKAMD_ERR_INVALID_ARG.  Synchronises
 * the stream (the analysis returns counts); apply does not. */
int kkamd_precond_create_lu(kkamd_precond_t** p, const kkamd_crs_t* L, const kkamd_crs_t* U, kkamd_stream_t stream);
int kkamd_precond_create_callback(kkamd_precond_t** p, kkamd_precond_fn fn, void* ctx);
/* Preconditioner::apply(X, Y, "N", alpha, beta) (KokkosSparse_Preconditioner.hpp:77-80); asynchronous on the stream */
int kkamd_precond_apply(kkamd_precond_t* p, const void* d_x, void* d_y, double alpha, double beta, int value_type, kkamd_stream_t stream);
int kkamd_precond_destroy(kkamd_precond_t* p);

/* ------------------------------------------------------------------------------------------------
 * Restarted GMRES with right preconditioning.  Replaces KokkosSparse::Experimental::gmres for a CrsMatrix
 * (sparse/src/KokkosSparse_gmres.hpp:58-158; handle sparse/src/KokkosSparse_gmres_handle.hpp:38-181; the loop
 * sparse/impl/KokkosSparse_gmres_impl.hpp:59-329, restated step for step on the host around the kernels of kk_gmres.hip).
 * The handle is the analogue of GMRESHandle plus this library's workspace: the basis V (n (m + 1) values), four work vectors, the
 * partial slabs of the deterministic reductions, the SpMV plan of the matrix last solved with; allocated at the first solve, kept while
 * n, m and the value type stay.  Not implemented: BSR matrices, complex scalars, the reference-side TPL binding.
 * ------------------------------------------------------------------------------------------------ */
typedef struct kkamd_gmres_handle kkamd_gmres_handle_t;
/* GMRESHandle::Ortho and ::Flag (gmres_handle.hpp:76-89) */
typedef enum { KKAMD_GMRES_CGS2 = 0, KKAMD_GMRES_MGS = 1 } kkamd_gmres_ortho;
typedef enum { KKAMD_GMRES_CONV = 0, KKAMD_GMRES_NO_CONV = 1, KKAMD_GMRES_LOA = 2, KKAMD_GMRES_NOT_RUN = 3 } kkamd_gmres_flag;
/* GMRESHandle(m = 50, tol = 1e-8, max_restart = 50) (gmres_handle.hpp:107-119): m <= 0 is KKAMD_ERR_INVALID_ARG with the reference's
 * text "gmres: Please choose restart size m greater than zero." */
int kkamd_gmres_create(kkamd_gmres_handle_t** handle, int64_t m, double tol, int64_t max_restart);
int kkamd_gmres_destroy(kkamd_gmres_handle_t* handle);
/* set_ortho / set_verbose / set_m / set_max_restart (gmres_handle.hpp:139-163) and this library's knobs:
 *   "ortho" 0 CGS2 (default), 1 MGS; "verbose" 0 / 1: the reference's lines on stdout; "m"; "max_restart";
 *   "fuse" 1 (default): the CGS2 step runs dot, fused update + dot, update + sum of squares, normalise (V read three times); 0: dot,
 *          update, dot, update + sum of squares, normalise (four times).  Same grouping and lane order: identical bits;
 *   "fuse_max_k" 1..64, default 17: with more columns than this the unfused pair runs whatever "fuse" says.  The default is the switch
 *          point measured on MI355X: beyond it the fused kernel's LDS tile and its accumulators cost more occupancy
 *          than the saved pass over V returns;
 *   "rows_per_group" rows per workgroup of the reductions: 0 (default) = max(1024, ceil(n / 1024) rounded up to 256), or a multiple of
 *          64 up to 2^24.  The bits of a result depend on n and this knob alone;
 *   "profile" 0 (default) / 1: four events per iteration on the stream; kkamd_gmres_export then gives "precond_ms", "spmv_ms" and
 *          "ortho_ms" (the orthogonalisation's kernels, without the copy of h), one value per iteration of the last solve. */
int kkamd_gmres_set(kkamd_gmres_handle_t* handle, const char* key, int64_t value);
int kkamd_gmres_set_tol(kkamd_gmres_handle_t* handle, double tol);
/* reset_handle(m, tol, max_restart) (gmres_handle.hpp:121-130): also ortho = CGS2, verbose off, results back to NotRun */
int kkamd_gmres_reset(kkamd_gmres_handle_t* handle, int64_t m, double tol, int64_t max_restart);
/* "num_iters" (-1 before a solve), "conv_flag" (a kkamd_gmres_flag, NOT_RUN before a solve), "cycles", of the last solve "host_syncs"
 * (stream synchronisations of the loop: one for the initial norms, one per CGS2 iteration -- j + 1 in MGS iteration j --, one per true
 * residual check) and "launches" (its own kernels, SpMV and preconditioner not counted), "plan_bytes" (HBM the handle keeps, the SpMV
 * plan included), the knobs, "last_fused" (1 when the last solve or kkamd_gmres_update ran the fused kernel),
 * "num_short_residuals" / "num_true_residuals" (entries of the exports below), "num_rows" (of the workspace) */
int kkamd_gmres_get(const kkamd_gmres_handle_t* handle, const char* key, int64_t* value);
/* "end_rel_res" (get_end_rel_res, -1 before a solve) | "tol" */
int kkamd_gmres_get_real(const kkamd_gmres_handle_t* handle, const char* key, double* value);
/* to a HOST buffer of `count` doubles: "short_residuals" (shortRelRes of every iteration of the last solve), "true_residuals" (relRes of
 * every evaluation: the initial one, then one per check), "hessenberg" (the un-rotated (m + 1) x m matrix of the last cycle, column-major),
 * "basis" (n x (m + 1), column-major, of the last cycle; columns the cycle did not reach hold older data); under "profile" the three
 * timing arrays (num_short_residuals entries each) */
int kkamd_gmres_export(const kkamd_gmres_handle_t* handle, const char* what, double* h_out, int64_t count);
/* gmres(handle, A, B, X, precond) (gmres.hpp:58-158).  d_b has A.num_rows entries, d_x A.num_cols (initial guess in, solution out); a
 * matrix that is not square is the reference's "KokkosSparse::gmres: Dimensions do not match: ..." (:110-116), KKAMD_ERR_INVALID_ARG.
 * Type pairs (F64,F64) and (F32,F32), else KKAMD_ERR_UNSUPPORTED.  precond: NULL or a right preconditioner, w = A (M v_j) and
 * Xiter = X + M (V y) through apply(alpha = 1, beta = 1) (gmres_impl.hpp:150-155,249-252).  KKAMD_ERR_NUMERIC with the reference's text
 * for a lucky breakdown without convergence (:219-223) and a NaN residual (:224-226; here also when the initial residual is NaN, which
 * the reference reports as NoConv).  Synchronises the stream, because it returns counts. */
int kkamd_gmres_solve(kkamd_gmres_handle_t* handle, const kkamd_crs_t* A, const void* d_b, void* d_x, kkamd_precond_t* precond, int vector_type,
                      kkamd_stream_t stream);
/* The building blocks, for a host with its own Arnoldi loop: V is n x k, column-major with column stride ldv >= n.
 * _dot: d_h[0..k) = V^T w -- KokkosBlas::gemv("C", one, V0j, Wj, zero, Hj) (gmres_impl.hpp:168).
 * _update: w_out = w_in + alpha * V h -- gemv("N") (:169; d_w_in NULL: w_out = alpha * V h; w_out may be w_in) -- and, when asked, from
 * the updated vector d_h2[0..k) = V^T w_out (gemv("C"), :173) and *d_sumsq = sum w_out^2 (nrm2 squared, :183).  With "fuse" 1, d_h2 given
 * and k <= "fuse_max_k" the update and the second product are one kernel.  Deterministic: the bits depend on n, k and "rows_per_group" alone.  Both
 * synchronise the stream (their partial slab is a temporary). */
int kkamd_gmres_dot(kkamd_gmres_handle_t* handle, int64_t n, int64_t k, const void* d_V, int64_t ldv, const void* d_w, void* d_h, int value_type,
                    kkamd_stream_t stream);
int kkamd_gmres_update(kkamd_gmres_handle_t* handle, int64_t n, int64_t k, double alpha, const void* d_V, int64_t ldv, const void* d_h,
                       const void* d_w_in, void* d_w_out, void* d_h2, void* d_sumsq, int value_type, kkamd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Threshold incomplete LU by fixed-point iteration (ParILUT).  Replaces KokkosSparse::Experimental::par_ilut_symbolic / par_ilut_numeric
 * (sparse/src/KokkosSparse_par_ilut.hpp:76-190, :207-380; handle sparse/src/KokkosSparse_par_ilut_handle.hpp:55-200; defaults
 * sparse/src/KokkosKernels_Handle.hpp:871-881; the loop sparse/impl/KokkosSparse_par_ilut_numeric_impl.hpp:724-876, restated step for step
 * around the kernels of kk_par_ilut.hip) for a square CrsMatrix whose rows are strictly ascending by column: int32 ordinals, int32 or int64
 * offsets (one type for A, L and U), F64 or F32 values.  L leaves with a unit diagonal LAST in every row, U with its diagonal FIRST, rows
 * ascending, as kkamd_precond_create_lu takes them.
 * Not implemented: async_update = true (recorded and without effect, as in the reference, whose numeric phase forces it off:
 * numeric_impl.hpp:740), BSR matrices, complex scalars, the reference-side TPL binding.
 * NaN values give an unspecified pattern (std::nth_element on NaN is undefined in the reference too).
 * Determinism: no floating-point atomics; the same bits on every run.  The bits depend on the lane count in use ("lanes_in_use": the knob
 * "lanes_per_row", or with 0 what covers the mean row of A) because the dot products of the L chain and the residual's row sums are reduced
 * across the lanes of a row; on nothing else.  The product L * U takes only its pattern from the SpGEMM: its values are summed in ascending k
 * by a kernel of this unit, so rows of L * U of any length (the SpGEMM adds rows of more than 256 entries with floating-point atomics) leave
 * the guarantee as it is.
 * ------------------------------------------------------------------------------------------------ */
typedef struct kkamd_par_ilut_handle kkamd_par_ilut_handle_t;
/* PAR_ILUTHandle(max_iter = 20, residual_norm_delta_stop = 1e-2, fill_in_limit = 0.75, async_update = false, verbose = false)
 * (par_ilut_handle.hpp:83-99; KokkosKernels_Handle.hpp:871-881).  max_iter < 0, fill_in_limit < 0 or a NaN: KKAMD_ERR_INVALID_ARG.  The
 * handle owns one SpGEMM handle and every workspace; workspaces only grow. */
int kkamd_par_ilut_create(kkamd_par_ilut_handle_t** handle, int64_t max_iter, double residual_norm_delta_stop, double fill_in_limit, int async_update,
                          int verbose);
int kkamd_par_ilut_destroy(kkamd_par_ilut_handle_t* handle);
/* par_ilut_symbolic(handle, A_rowmap, A_entries, L_rowmap, U_rowmap) (par_ilut.hpp:76-190; symbolic_impl.hpp:36-93): row i of L gets
 * 1 + #{col < i} entries, row i of U 1 + #{col > i}; both row maps (num_rows + 1 offsets) are scanned; nnzL, nnzU and num_rows go to the
 * handle.  The graph is validated on the host before anything is indexed by it: a row map that does not ascend, a column outside
 * [0, num_rows), a row that is not strictly ascending by column -- KKAMD_ERR_INVALID_ARG naming the smallest offending row; the last one
 * carries the text the reference only asserts inside a kernel (numeric_impl.hpp:306, "is your A matrix sorted?").  Synchronises. */
int kkamd_par_ilut_symbolic(kkamd_par_ilut_handle_t* handle, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries, void* d_L_row_map,
                            void* d_U_row_map, int offset_type, kkamd_stream_t stream);
/* par_ilut_numeric(handle, A_rowmap, A_entries, A_values, L_rowmap, L_entries, L_values, U_rowmap, U_entries, U_values) (par_ilut.hpp:207-380;
 * numeric_impl.hpp:724-876).  The sizes of the factors depend on the data (the reference resizes the caller's views every iteration), so
 * the factors stay in the handle: the call writes the two FINAL row maps, "nnzL_out" / "nnzU_out" give the sizes and
 * kkamd_par_ilut_copy_factors the entries and values.  The symbolic row maps are kept by the handle, so the call may be repeated with new
 * values.  Before a completed symbolic call: KKAMD_ERR_STATE; another value type: KKAMD_ERR_UNSUPPORTED; num_rows or offset_type other than
 * the symbolic call's: KKAMD_ERR_INVALID_ARG.  Synchronises the stream (sizes come back every iteration: "host_syncs"). */
int kkamd_par_ilut_numeric(kkamd_par_ilut_handle_t* handle, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries, const void* d_A_values,
                           void* d_L_row_map, void* d_U_row_map, int offset_type, int value_type, kkamd_stream_t stream);
/* The factors of the last numeric call, of its value type, on the stream.  A capacity below "nnzL_out" / "nnzU_out": KKAMD_ERR_INVALID_ARG
 * with the true count, nothing written.  Before a completed numeric call: KKAMD_ERR_STATE. */
int kkamd_par_ilut_copy_factors(kkamd_par_ilut_handle_t* handle, int32_t* d_L_entries, void* d_L_values, int64_t L_capacity, int32_t* d_U_entries,
                                void* d_U_values, int64_t U_capacity, kkamd_stream_t stream);
/* set_max_iter / set_residual_norm_delta_stop / set_fill_in_limit / set_async_update / set_verbose (par_ilut_handle.hpp:140-160):
 *   "max_iter" >= 0; "residual_norm_delta_stop" (<= 0: no residual is computed and max_iter iterations run); "fill_in_limit" >= 0;
 *   "async_update" 0 / 1, recorded, without effect; "verbose" 0 / 1: the reference's lines on stdout, from the host;
 *   "lanes_per_row" 0 (default: what covers the mean row of A) or a power of two, 1..64;
 *   "profile" 0 (default) / 1: the numeric phase synchronises the stream after every step and reads the host clock; kkamd_par_ilut_get_real
 *          then gives "product_ms", "candidates_ms", "transpose_ms", "sweep_ms", "select_ms", "filter_ms" and "residual_ms", each summed
 *          over the iterations of the last numeric call (a measurement aid: it changes no result).
 * Values outside these ranges and unknown keys: KKAMD_ERR_INVALID_ARG. */
int kkamd_par_ilut_set(kkamd_par_ilut_handle_t* handle, const char* key, double value);
/* "num_iters" (get_num_iters, -1 before a numeric call), "nnzL", "nnzU", "num_rows" (of the symbolic call), "nnzL_out", "nnzU_out",
 * "symbolic_complete", "numeric_complete", "max_iter", "async_update", "verbose", "lanes_per_row", "lanes_in_use",
 * "stage_entries_per_lane", "plan_bytes" (HBM the handle holds, the SpGEMM handle's own not counted); of the last numeric call "host_syncs"
 * (the synchronisations this unit issues itself: per iteration one for the candidate counts, one for the filtered counts and thresholds,
 * one for the residual -- and one at the end; kkamd_spgemm_symbolic and kkamd_transpose synchronise inside in addition, and so does every
 * hipMalloc / hipFree of a workspace that grows inside the loop: none of these is counted) and
 * "launches" (its own kernels and scans; SpGEMM, transpose and sort not counted) and "max_product_row" (the longest row of L * U met) */
int kkamd_par_ilut_get(const kkamd_par_ilut_handle_t* handle, const char* key, int64_t* value);
/* "end_rel_res" (get_end_rel_res, -1 before a numeric call), the last "l_threshold" / "u_threshold", "residual_norm_delta_stop",
 * "fill_in_limit", the seven step times of "profile" */
int kkamd_par_ilut_get_real(const kkamd_par_ilut_handle_t* handle, const char* key, double* value);
/* The steps of one iteration on caller-held device arrays, so that each can be tested alone.  The arrays are taken as the numeric phase holds
 * them (sorted rows, columns in range, L's unit diagonal last, U's diagonal first) and are not validated.  They run with "lanes_per_row"
 * lanes (0: 8) and synchronise the stream.
 * _add_candidates (numeric_impl.hpp:129-328): L_new / U_new from A, the old L and U and LU = L * U.  Always writes the two row maps and
 *   *nnzLn / *nnzUn; with both entry arrays NULL it stops there (the sizing call); a capacity too small is KKAMD_ERR_INVALID_ARG with the counts.
 * _sweep (:354-458, compute_l_u_factors with async_update == false): renews L_values and U_values in place against the frozen Ut.
 * _select (:480-494): the value of rank `rank` (0-based, ascending) among |values| into the device scalar d_threshold, by radix select;
 *   exactly the order statistic (ties, zeros, -0.0, denormals, Inf).
 * _filter (:496-597): keeps |v| >= *d_threshold or the diagonal, in stored order; sizing call with d_O_entries NULL as above.
 * _residual (:602-668): sqrt(sum over A's pattern of (a - lu)^2), the sum in the value type, the square root on the host. */
int kkamd_par_ilut_add_candidates(kkamd_par_ilut_handle_t* handle, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries,
                                  const void* d_A_values, const void* d_L_row_map, const int32_t* d_L_entries, const void* d_L_values,
                                  const void* d_U_row_map, const int32_t* d_U_entries, const void* d_U_values, const void* d_LU_row_map,
                                  const int32_t* d_LU_entries, const void* d_LU_values, int64_t nnzLU, void* d_Ln_row_map, int32_t* d_Ln_entries,
                                  void* d_Ln_values, int64_t Ln_capacity, void* d_Un_row_map, int32_t* d_Un_entries, void* d_Un_values,
                                  int64_t Un_capacity, int64_t* nnzLn, int64_t* nnzUn, int offset_type, int value_type, kkamd_stream_t stream);
int kkamd_par_ilut_sweep(kkamd_par_ilut_handle_t* handle, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries, const void* d_A_values,
                         const void* d_L_row_map, const int32_t* d_L_entries, void* d_L_values, const void* d_U_row_map, const int32_t* d_U_entries,
                         void* d_U_values, const void* d_Ut_row_map, const int32_t* d_Ut_entries, const void* d_Ut_values, int offset_type,
                         int value_type, kkamd_stream_t stream);
int kkamd_par_ilut_select(kkamd_par_ilut_handle_t* handle, int64_t count, const void* d_values, int64_t rank, void* d_threshold, int value_type,
                          kkamd_stream_t stream);
int kkamd_par_ilut_filter(kkamd_par_ilut_handle_t* handle, int64_t num_rows, const void* d_I_row_map, const int32_t* d_I_entries, const void* d_I_values,
                          const void* d_threshold, void* d_O_row_map, int32_t* d_O_entries, void* d_O_values, int64_t O_capacity, int64_t* nnz_out,
                          int offset_type, int value_type, kkamd_stream_t stream);
int kkamd_par_ilut_residual(kkamd_par_ilut_handle_t* handle, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries, const void* d_A_values,
                            const void* d_LU_row_map, const int32_t* d_LU_entries, const void* d_LU_values, double* residual_norm, int offset_type,
                            int value_type, kkamd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Distance-2 maximal independent set, MIS-2 aggregation and explicit graph coarsening.  Replaces KokkosGraph::graph_d2_mis,
 * graph_mis2_coarsen, graph_mis2_aggregate (graph/src/KokkosGraph_MIS2.hpp:24-87; native implementation
 * graph/impl/KokkosGraph_Distance2MIS_impl.hpp: MIS2_FAST :30-470, MIS2_QUALITY :472-793, the aggregation :795-1114) and
 * KokkosGraph::Experimental::graph_explicit_coarsen / graph_explicit_coarsen_with_inverse_map
 * (graph/src/KokkosGraph_ExplicitCoarsening.hpp:35-92) for a symmetric CRS graph: int32 ordinals, int32 or int64 offsets, no values.
 * The graph is borrowed.  Handle-less, as the reference's are free functions.  Columns >= num_verts are ignored everywhere; self-loops
 * are harmless.  Symmetry is the caller's contract, as in the reference; it is not checked up front.
 *
 * The results are the reference's, exactly, and functions of the graph alone.  Statuses are 32-bit unsigned, IN_SET = 0,
 * OUT_SET = 0xFFFFFFFF, nvBits = the bit length of num_verts + 1.  MIS2_FAST: in round r = 0, 1, ... every undecided row i takes
 *     status(i) = (i + 1) | (hash(hash(i) ^ hash(r)) << nvBits)          (modulo 2^32; decremented when it equals OUT_SET)
 * where, for a 32-bit unsigned v taken into the 64-bit unsigned x (xorshiftHash<uint32_t>, common/src/KokkosKernels_SimpleUtils.hpp:377-385),
 *     x ^= x >> 12;  x ^= x << 25;  x ^= x >> 27;  hash(v) = the low 32 bits of ((x * 2685821657736338717 - 1) >> 16)   (modulo 2^64);
 * every live column takes the minimum status over itself and its neighbours, IN_SET counting as OUT_SET; an undecided row becomes OUT_SET
 * when a column of its closed neighbourhood is OUT_SET, else IN_SET when all of them carry its own status.  Decided rows and OUT_SET
 * columns leave the work lists.  MIS2_QUALITY: the same round with the fixed statuses
 *     status(i) = (i + 1) + ((uint32)(score(i) * (float)((1 << (32 - nvBits)) - 2)) << nvBits),
 *     score(i) = (float)(deg(i) - minDeg) * (1.f / (float)(maxDeg - minDeg))    in fp32, deg = the row's stored length;
 * when all degrees are equal the reference divides by zero and casts a NaN: here score = 0 (a documented difference,
 * like the two below: the report of a graph that is not symmetric, and the defined order of the rows without compress).
 *
 * Validation: one pass checks that row_map ascends and that no entry is negative: KKAMD_ERR_INVALID_ARG naming the smallest offending
 * row.  On a symmetric graph every round decides at least the undecided row of smallest status; a round that decides no row returns
 * KKAMD_ERR_INVALID_ARG "graph is not symmetric" where the reference would not return.  No input makes the host loop run without bound.
 *
 * stats: NULL, or 8 values: [0] rounds of the first MIS-2, [1] rounds of the masked MIS-2 (0 without one), [2] host synchronisations,
 * [3] kernel launches, [4] primary aggregates, [5] secondary aggregates, [6] vertices still unlabelled before phase 3, [7] bytes of
 * scratch.  Host synchronisations: one per round (the surviving lengths) plus a constant per call:
 *     graph_d2_mis, graph_mis2_coarsen: 2 + rounds;   graph_mis2_aggregate: 3 + rounds + masked rounds.
 * Kernel launches per round: 4 (column statuses, row decisions, one scan of the workgroup counts, the move; 6 with more than 2048
 * workgroups).  The knob kkamd_set_default("mis2_lanes_per_vertex", 0 | 1 | 2 | ... | 64) sets the lanes per work-list vertex, 0 (default)
 * = the smallest power of two that gives a lane at most about four entries of the mean closed neighbourhood.  No output depends on it.
 * num_verts == 0: an empty set, zero aggregates, no launch.
 * ------------------------------------------------------------------------------------------------ */
/* KokkosGraph::MIS2_Algorithm (KokkosGraph_MIS2.hpp:24), in the reference's order */
typedef enum { KKAMD_MIS2_QUALITY = 0, KKAMD_MIS2_FAST = 1 } kkamd_mis2_algorithm;
/* graph_d2_mis(rowmap, colinds, algo) (KokkosGraph_MIS2.hpp:31-49): the set in ascending vertex order into d_mis (num_verts int32 of
 * room), its size into *num_in_set.  Any other algorithm: KKAMD_ERR_INVALID_ARG with the reference's "graph_d2_mis: invalid algorithm". */
int kkamd_graph_d2_mis(int64_t num_verts, const void* d_row_map, int offset_type, const int32_t* d_entries, int algorithm, int32_t* d_mis,
                       int64_t* num_in_set, int64_t* stats, kkamd_stream_t stream);
/* secondary == 0: graph_mis2_coarsen(rowmap, colinds, numClusters) (KokkosGraph_MIS2.hpp:51-64); != 0: graph_mis2_aggregate
 * (:66-79).  d_labels: num_verts int32.  Phase 1: MIS2_FAST, aggregate a = the a-th root in ascending order and its neighbours.  Phase 2
 * (secondary only): the masked MIS2_FAST over the unlabelled vertices; a candidate with at least 3 unlabelled vertices in its closed
 * neighbourhood becomes an aggregate, the ids continuing in ascending candidate order (a scan, no atomic counter).  Phase 3, from a
 * frozen copy of the labels: every non-root vertex walks its entries in stored order, tracks up to 8 distinct neighbouring aggregates,
 * stops at the ninth, and moves by: adjacent to a root > connectivity > smaller size, the first best winning.  On a symmetric graph every
 * vertex ends labelled in [0, *num_aggregates). */
int kkamd_graph_mis2_aggregate(int64_t num_verts, const void* d_row_map, int offset_type, const int32_t* d_entries, int secondary,
                               int32_t* d_labels, int64_t* num_aggregates, int64_t* stats, kkamd_stream_t stream);
/* graph_explicit_coarsen(fineRowmap, fineEntries, labels, numCoarseVerts, coarseRowmap, coarseEntries, compress) and
 * graph_explicit_coarsen_with_inverse_map (KokkosGraph_ExplicitCoarsening.hpp:35-92).  Coarse row c holds the labels != c of the in-range
 * neighbours of cluster c's vertices.  compress != 0: sorted and merged, exactly the reference's result.  compress == 0: the reference's
 * order and duplicates depend on atomics and a 512-slot hash table; here the row is defined: the cluster's vertices in ascending order,
 * their entries in stored order, every cross-cluster entry kept -- the same set per row, never more than nnz entries.
 * d_coarse_row_map: num_coarse + 1 offsets of the fine offset type; d_coarse_entries: `capacity` int32 of room.  *coarse_nnz is the
 * entry count; capacity < *coarse_nnz returns KKAMD_ERR_INVALID_ARG with the true count and writes nothing, so a first call with
 * capacity 0 sizes the second.  d_inverse_offsets (num_coarse + 1) / d_inverse_labels (num_verts): NULL, or the vertices grouped by
 * cluster, ascending inside a cluster (the reference leaves that order to an atomic).  A label outside [0, num_coarse):
 * KKAMD_ERR_INVALID_ARG naming the smallest offending vertex.  Synchronises the stream. */
int kkamd_graph_explicit_coarsen(int64_t num_verts, const void* d_row_map, int offset_type, const int32_t* d_entries, const int32_t* d_labels,
                                 int64_t num_coarse, int compress, void* d_coarse_row_map, int32_t* d_coarse_entries, int64_t capacity,
                                 int64_t* coarse_nnz, int32_t* d_inverse_offsets, int32_t* d_inverse_labels, kkamd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Helpers either side of the path (KokkosSparse::sort_crs_matrix, sparse/src/KokkosSparse_SortCrs.hpp:43-120;
 * kk_exclusive_parallel_prefix_sum, common/src/KokkosKernels_SimpleUtils.hpp:86-135) and the synthetic
 * inputs of the benchmark configurations, generated in place in HBM
 * (test_common/KokkosKernels_Test_Structured_Matrix.hpp, BC = 1 on every face).
 * ------------------------------------------------------------------------------------------------ */
int kkamd_sort_crs(int64_t num_rows, const void* d_row_map, int32_t* d_entries, void* d_values, int offset_type,
                   int value_type, kkamd_stream_t stream);

/* KokkosSparse::sort_and_merge_matrix (sparse/src/KokkosSparse_SortCrs.hpp:304-363): sort every row by column and
 * collapse runs of equal columns into one entry whose value is the sum of the run (left to right).  Two calls:
 *   1. d_entries_out == NULL: sorts (d_entries, d_values) IN PLACE, writes the merged row_map to d_row_map_out
 *      (num_rows + 1 offsets) and the merged entry count to *nnz_out;
 *   2. d_entries_out / d_values_out sized *nnz_out: fills them (the inputs must be the ones sorted by call 1).
 * d_values may be NULL (graph only). */
int kkamd_sort_and_merge(int64_t num_rows, const void* d_row_map, int32_t* d_entries, void* d_values, int offset_type,
                         int value_type, void* d_row_map_out, int32_t* d_entries_out, void* d_values_out, int64_t* nnz_out,
                         kkamd_stream_t stream);

/* KokkosSparse::Impl::transpose_matrix (sparse/src/KokkosSparse_Utils.hpp:338-400): CRS of the transpose into
 * preallocated d_t_row_map (num_cols + 1), d_t_entries / d_t_values (nnz).  Rows of the result are column-sorted (the
 * reference leaves the order to its atomics).  d_values may be NULL (transpose_graph, :402-440). */
int kkamd_transpose(int64_t num_rows, int64_t num_cols, int64_t nnz, const void* d_row_map, const int32_t* d_entries,
                    const void* d_values, int offset_type, int value_type, void* d_t_row_map, int32_t* d_t_entries,
                    void* d_t_values, kkamd_stream_t stream);
int kkamd_exclusive_scan(void* d_data, int64_t n, int offset_type, kkamd_stream_t stream);

/* dim = 2 or 3; stencil 0 = FD (5/7-pt), 1 = FE (9/27-pt).  With d_entries == NULL only row_map is
 * filled (and *nnz returned), so the caller can size entries/values. */
int kkamd_gen_laplace(int dim, int stencil, int64_t nx, int64_t ny, int64_t nz, void* d_row_map, int32_t* d_entries,
                      void* d_values, int offset_type, int value_type, int64_t* nnz, kkamd_stream_t stream);
/* One contiguous row slab [row_begin, row_begin+row_count) of the same matrix: local row_map (starting
 * at 0), GLOBAL column indices -- the per-GPU piece of the 1-D row partition. */
int kkamd_gen_laplace_rows(int dim, int stencil, int64_t nx, int64_t ny, int64_t nz, int64_t row_begin,
                           int64_t row_count, void* d_row_map, int32_t* d_entries, void* d_values, int offset_type,
                           int value_type, int64_t* nnz, kkamd_stream_t stream);

/* Device streaming-read microbenchmark (bench tooling): reads `bytes` from d_data with `loads` independent
 * 16-byte loads in flight per lane; the measured HBM read ceiling quoted beside roofline fractions. */
int kkamd_bench_read(const void* d_data, int64_t bytes, int loads, int nontemporal, int persistent, void* d_out,
                     kkamd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KKAMD_H */
