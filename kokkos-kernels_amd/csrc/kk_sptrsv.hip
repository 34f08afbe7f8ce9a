// kk_sptrsv.hip -- level-scheduled sparse triangular solve: KokkosSparse::sptrsv_symbolic / sptrsv_solve
// (sparse/src/KokkosSparse_sptrsv.hpp:54-122,268-411) for a square CRS triangle with its diagonal stored.
//
// Symbolic phase, on the device.  The reference copies the graph to the host and finds the level sets in one sequential loop over
// the entries (sparse/impl/KokkosSparse_sptrsv_symbolic_impl.hpp:156-214, upper :569-640).  Here:
//   1. one pass validates every row (columns in range, on the right side of the diagonal, exactly one diagonal entry), records the
//      diagonal's position inside the row and the row's number of off-diagonal entries (its in-degree), and queues the rows without
//      any: they are level 1;
//   2. the graph is transposed (kkamd_transpose, values NULL): row j of the transpose lists the rows that wait for x[j];
//   3. frontiers are peeled, one launch per level: every row of the level decrements the counter of each row that waits for it
//      (integer atomic); a row whose counter reaches zero gets level + 1 and joins the queue.  level(i) = 1 + max level(col) follows
//      because the last column to be solved is the one that brings the counter to zero;
//   4. the queue holds the rows level by level already; each level's piece is sorted ascending (kkamd_sort_crs with the level offsets
//      as row_map).
// level_list is a function of the graph alone, the other two arrays are functions of level_list: the order of the atomics changes
// nothing.  One host synchronisation per level (the queue's tail); at most num_rows levels.
// The analysis fills a kk::LevelSchedule (kk_levels.h) through analyse_levels, which ILU(k) calls too (kk_spiluk.hip); the launches of one
// solve are built from it and the knobs.
//
// Solve phase.  One launch per level: a group of LPR lanes owns one row of the level's list, strides over its entries, skips the
// diagonal position, reduces with kk::group_sum (fixed order: the same bits on every run) and its first lane writes x[row].  Runs of
// consecutive narrow levels may be chained into one single-workgroup launch with __syncthreads() between the levels.
// No work-item ever waits on another workgroup: every dependency between workgroups is a kernel boundary on the stream.
#include "kk_levels.h"
#include <climits>
#include <new>

namespace kk {

constexpr unsigned long long kNoError = ~0ull;
enum { kErrRowMap = 0, kErrColumn = 1, kErrSide = 2, kErrNoDiag = 3, kErrManyDiag = 4, kErrNone = 7 };
constexpr int kSymLanes = 8;   // lanes per row of the analysis kernels

// ctr[0] queue tail, ctr[1] entries of the queued rows so far, ctr[2] min over the offending rows of row * 8 + kind
template <class OffT>
__global__ __launch_bounds__(kBlock) void sptrsv_validate_kernel(int64_t n, int lower, const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                                 int32_t* __restrict__ diagpos, int32_t* __restrict__ indeg,
                                                                 int32_t* __restrict__ level_list, int32_t* __restrict__ queue,
                                                                 unsigned long long* __restrict__ ctr) {
  const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kSymLanes;
  const int lane  = threadIdx.x & (kSymLanes - 1);
  const bool valid = r < n;
  int kind = kErrNone, ndiag = 0, dpos = -1;
  int64_t len = 0;
  if (valid) {
    const int64_t s = (int64_t)rm[r], e = (int64_t)rm[r + 1];
    len = e - s;
    if (s < 0 || len < 0 || len > (int64_t)INT32_MAX) { kind = kErrRowMap; len = 0; }
    for (int64_t j = s + lane; j < s + len; j += kSymLanes) {
      const int64_t c = ent[j];
      if (c < 0 || c >= n) { if (kErrColumn < kind) kind = kErrColumn; }
      else if (lower ? c > r : c < r) { if (kErrSide < kind) kind = kErrSide; }
      else if (c == r) { ++ndiag; dpos = (int)(j - s); }
    }
  }
  for (int o = kSymLanes >> 1; o > 0; o >>= 1) {           // every lane of the wave takes part, rows past the end included
    const int k2 = __shfl_xor(kind, o, 64), n2 = __shfl_xor(ndiag, o, 64), d2 = __shfl_xor(dpos, o, 64);
    kind = k2 < kind ? k2 : kind; ndiag += n2; dpos = d2 > dpos ? d2 : dpos;
  }
  if (!valid || lane != 0) return;
  if (kind == kErrNone && ndiag == 0) kind = kErrNoDiag;
  if (kind == kErrNone && ndiag > 1) kind = kErrManyDiag;
  if (kind != kErrNone) { atomicMin(&ctr[2], (unsigned long long)r * 8ull + (unsigned long long)kind); return; }
  diagpos[r] = dpos;
  indeg[r]   = (int32_t)(len - 1);
  if (len == 1) {
    level_list[r] = 1;
    queue[atomicAdd(&ctr[0], 1ull)] = (int32_t)r;
    atomicAdd(&ctr[1], 1ull);
  }
}

// rows queue[head .. head + cnt) have level next_level - 1.  queue is read there and appended to behind its tail: no __restrict__.
template <class OffT>
__global__ __launch_bounds__(kBlock) void sptrsv_peel_kernel(int32_t* queue, int64_t head, int64_t cnt, const OffT* __restrict__ t_rm,
                                                             const int32_t* __restrict__ t_ent, const OffT* __restrict__ rm,
                                                             int32_t* __restrict__ indeg, int32_t* __restrict__ level_list, int32_t next_level,
                                                             unsigned long long* __restrict__ ctr) {
  const int64_t g = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kSymLanes;
  const int lane  = threadIdx.x & (kSymLanes - 1);
  if (g >= cnt) return;
  const int32_t j = queue[head + g];
  const int64_t e = (int64_t)t_rm[j + 1];
  for (int64_t p = (int64_t)t_rm[j] + lane; p < e; p += kSymLanes) {
    const int32_t i = t_ent[p];
    if (i == j) continue;
    if (atomicAdd(&indeg[i], -1) == 1) {
      level_list[i] = next_level;
      queue[atomicAdd(&ctr[0], 1ull)] = i;
      atomicAdd(&ctr[1], (unsigned long long)((int64_t)rm[i + 1] - (int64_t)rm[i]));
    }
  }
}

template <class OffT>
static int analyse_levels_typed(LevelSchedule* s, int64_t n, int lower, const OffT* rm, const int32_t* ent, int offset_type, hipStream_t st,
                                DevBuf* level_b, DevBuf* diag_b) {
  DevBuf grouped_b, off_b, indeg_b, ctr_b, trm_b, tent_b;
  KK_HIP(level_b->alloc(sizeof(int32_t) * (size_t)n));
  KK_HIP(grouped_b.alloc(sizeof(int32_t) * (size_t)n));
  KK_HIP(diag_b->alloc(sizeof(int32_t) * (size_t)n));
  KK_HIP(indeg_b.alloc(sizeof(int32_t) * (size_t)n));
  KK_HIP(ctr_b.alloc(sizeof(unsigned long long) * 3));
  int32_t *level_list = level_b->as<int32_t>(), *queue = grouped_b.as<int32_t>(), *indeg = indeg_b.as<int32_t>(), *diagpos = diag_b->as<int32_t>();
  unsigned long long* ctr = ctr_b.as<unsigned long long>();
  KK_HIP(hipMemsetAsync(ctr, 0, 16, st));
  KK_HIP(hipMemsetAsync(ctr + 2, 0xFF, 8, st));
  KK_LAUNCH((sptrsv_validate_kernel<OffT>), (unsigned)ceil_div(n * kSymLanes, kBlock), kBlock, 0, st, n, lower, rm, ent, diagpos, indeg,
            level_list, queue, ctr);
  KK_LAUNCH_CHECK();
  unsigned long long hc[3] = {0, 0, 0};
  OffT h_nnz = 0;
  KK_HIP(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, st));
  KK_HIP(hipMemcpyAsync(&h_nnz, rm + n, sizeof(OffT), hipMemcpyDeviceToHost, st));
  KK_HIP(hipStreamSynchronize(st));
  if (hc[2] != kNoError) {
    static const char* const what[] = {"its row_map offsets are not ascending (or it has more than 2^31 - 1 entries)",
                                       "a column is outside [0, num_rows)", "", "it has no diagonal entry", "it has more than one diagonal entry"};
    const long long row = (long long)(hc[2] >> 3);
    const int kind = (int)(hc[2] & 7);
    if (kind == kErrSide)
      return fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_symbolic: row %lld: an entry lies %s the diagonal of a%s triangular matrix", row,
                  lower ? "above" : "below", lower ? " lower" : "n upper");
    return fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_symbolic: row %lld: %s", row, what[kind]);
  }
  const int64_t nnz = (int64_t)h_nnz;
  int64_t head = 0, tail = (int64_t)hc[0];
  if (tail == 0) return fail(KKAMD_ERR_STATE, "kkamd_sptrsv_symbolic: no row without off-diagonal entries (internal error)");
  if (tail < n) {
    // row j of the transpose: the rows that read x[j]
    KK_HIP(trm_b.alloc(sizeof(OffT) * (size_t)(n + 1)));
    KK_HIP(tent_b.alloc(sizeof(int32_t) * (size_t)nnz));
    const int rc = kkamd_transpose(n, n, nnz, rm, ent, nullptr, offset_type, KKAMD_F64, trm_b.p, tent_b.as<int32_t>(), nullptr,
                                   reinterpret_cast<kkamd_stream_t>(st));
    if (rc) return rc;
  }
  const OffT* t_rm = trm_b.as<OffT>();
  const int32_t* t_ent = tent_b.as<int32_t>();
  std::vector<int64_t> level_off(1, 0), level_entries;
  unsigned long long entries_before = 0;
  for (int64_t lvl = 1;; ++lvl) {                            // at most n levels: every level holds at least one row
    level_off.push_back(tail);
    level_entries.push_back((int64_t)(hc[1] - entries_before));
    entries_before = hc[1];
    if (tail >= n) break;
    if (lvl >= n) return fail(KKAMD_ERR_STATE, "kkamd_sptrsv_symbolic: more levels than rows (internal error)");
    const int64_t cnt = tail - head;
    KK_LAUNCH((sptrsv_peel_kernel<OffT>), (unsigned)ceil_div(cnt * kSymLanes, kBlock), kBlock, 0, st, queue, head, cnt, t_rm, t_ent, rm, indeg, level_list, (int32_t)(lvl + 1), ctr);
    KK_LAUNCH_CHECK();
    KK_HIP(hipMemcpyAsync(hc, ctr, 16, hipMemcpyDeviceToHost, st));
    KK_HIP(hipStreamSynchronize(st));
    if ((int64_t)hc[0] <= tail) return fail(KKAMD_ERR_STATE, "kkamd_sptrsv_symbolic: level %lld released no row (internal error)", (long long)lvl);
    head = tail;
    tail = (int64_t)hc[0];
  }
  trm_b.reset(); tent_b.reset(); indeg_b.reset(); ctr_b.reset();
  const int64_t L = (int64_t)level_off.size() - 1;
  KK_HIP(off_b.alloc(sizeof(int64_t) * (size_t)(L + 1)));
  KK_HIP(hipMemcpyAsync(off_b.p, level_off.data(), sizeof(int64_t) * (size_t)(L + 1), hipMemcpyHostToDevice, st));
  KK_HIP(hipStreamSynchronize(st));
  // ascending row order inside every level
  const int rc = kkamd_sort_crs(L, off_b.p, queue, nullptr, KKAMD_I64, KKAMD_F64, reinterpret_cast<kkamd_stream_t>(st));
  if (rc) return rc;
  KK_HIP(hipStreamSynchronize(st));
  s->d_grouped   = (int32_t*)grouped_b.release();
  s->d_level_off = (int64_t*)off_b.release();
  s->level_off.swap(level_off);
  s->level_entries.swap(level_entries);
  for (int64_t l = 0; l < L; ++l) {
    const int64_t w = s->level_off[l + 1] - s->level_off[l];
    if (w > s->max_level_rows) s->max_level_rows = w;
  }
  return KKAMD_OK;
}

int analyse_levels(LevelSchedule* s, int64_t n, int lower, const void* row_map, const int32_t* entries, int offset_type, hipStream_t st,
                   DevBuf* level_list, DevBuf* diagpos) {
  if (n == 0) {
    KK_HIP(hipStreamSynchronize(st));
    s->level_off.assign(1, 0);
    return KKAMD_OK;
  }
  return offset_type == KKAMD_I64 ? analyse_levels_typed<int64_t>(s, n, lower, (const int64_t*)row_map, entries, offset_type, st, level_list, diagpos)
                                  : analyse_levels_typed<int32_t>(s, n, lower, (const int32_t*)row_map, entries, offset_type, st, level_list, diagpos);
}

// One row per group of lpr lanes (a power of two, 1..64).  x of the row's off-diagonal columns was written by an earlier launch, or
// by this workgroup before its last barrier.  b may be x: b[row] is read by the lane that writes x[row].  Neither pointer is
// const / __restrict__, so x is read with ordinary vector loads.
template <class OffT, class VT>
__device__ __forceinline__ void sptrsv_row(bool valid, const int32_t* __restrict__ rows, int64_t g, int lane, int lpr, const OffT* __restrict__ rm,
                                           const int32_t* __restrict__ ent, const VT* __restrict__ val, const int32_t* __restrict__ diagpos,
                                           const VT* b, VT* x) {
  VT acc = VT(0);
  int32_t row = 0;
  int64_t dp = 0;
  if (valid) {
    row = rows[g];
    const int64_t s = (int64_t)rm[row], e = (int64_t)rm[row + 1];
    dp = s + diagpos[row];
    for (int64_t j = s + lane; j < e; j += lpr)              // rows longer than one pass loop
      if (j != dp) acc += val[j] * x[ent[j]];
  }
  acc = group_sum(acc, lpr);
  if (valid && lane == 0) x[row] = (b[row] - acc) / val[dp];
}

template <class OffT, class VT>
__global__ __launch_bounds__(kBlock) void sptrsv_level_kernel(const int32_t* __restrict__ rows, int64_t cnt, int lpr, int lpr_shift,
                                                              const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                              const VT* __restrict__ val, const int32_t* __restrict__ diagpos, const VT* b, VT* x) {
  const int64_t g = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> lpr_shift;
  sptrsv_row<OffT, VT>(g < cnt, rows, g, threadIdx.x & (lpr - 1), lpr, rm, ent, val, diagpos, b, x);
}

// levels [first, first + nlev) in one workgroup; the barrier's workgroup-scope ordering is all x needs between them
template <class OffT, class VT>
__global__ __launch_bounds__(kBlock) void sptrsv_chain_kernel(const int32_t* __restrict__ grouped, const int64_t* __restrict__ level_off, int first,
                                                              int nlev, int lpr, int lpr_shift, const OffT* __restrict__ rm,
                                                              const int32_t* __restrict__ ent, const VT* __restrict__ val,
                                                              const int32_t* __restrict__ diagpos, const VT* b, VT* x) {
  const int lane = threadIdx.x & (lpr - 1), grp = threadIdx.x >> lpr_shift, ngrp = kBlock >> lpr_shift;
  for (int l = first; l < first + nlev; ++l) {
    const int64_t beg = level_off[l], cnt = level_off[l + 1] - beg;
    for (int64_t base = 0; base < cnt; base += ngrp)         // uniform trip count: every lane reaches the reduction
      sptrsv_row<OffT, VT>(base + grp < cnt, grouped + beg, base + grp, lane, lpr, rm, ent, val, diagpos, b, x);
    __syncthreads();
  }
}

}  // namespace kk

struct kkamd_sptrsv_handle {
  int algorithm = 0, lower = 1;
  int64_t nrows = 0;
  bool symbolic_complete = false;
  kk::LevelSchedule sched;
  int32_t *d_level_list = nullptr, *d_diagpos = nullptr;

  void clear_symbolic() {
    symbolic_complete = false;
    sched.clear();
    if (d_level_list) (void)hipFree(d_level_list);
    if (d_diagpos) (void)hipFree(d_diagpos);
    d_level_list = d_diagpos = nullptr;
  }
};

namespace kk {

// The launches of one solve.  Lanes per row: what covers the mean row length (diagonal included) of the launch's levels.  On the lower
// triangle of the 27-point lattice (13.9 entries per row) 16 lanes measured 5 % faster than 8
static void sptrsv_build_plan(kkamd_sptrsv_handle* h) {
  build_plan(&h->sched, h->algorithm == KKAMD_SPTRSV_SEQLVLSCHD_TP1CHAIN && h->sched.chain_rows > 0, [h](int64_t entries, int64_t rows) {
    if (h->algorithm == KKAMD_SPTRSV_SEQLVLSCHD_RP) return 1;
    if (h->sched.lanes_per_row) return h->sched.lanes_per_row;
    return pow2_covering(rows > 0 ? ceil_div(entries, rows) : 1);
  });
}

template <class OffT, class VT>
static int sptrsv_solve_typed(const kkamd_sptrsv_handle* h, const OffT* rm, const int32_t* ent, const VT* val, const VT* b, VT* x, hipStream_t st) {
  const LevelSchedule& s = h->sched;
  for (const LevelLaunch& q : s.plan) {
    const int sh = log2i(q.lpr);
    if (q.chain) {
      KK_LAUNCH((sptrsv_chain_kernel<OffT, VT>), 1u, kBlock, 0, st, (const int32_t*)s.d_grouped, (const int64_t*)s.d_level_off, q.first, q.nlev, q.lpr,
                sh, rm, ent, val, (const int32_t*)h->d_diagpos, b, x);
    } else {
      const int64_t beg = s.level_off[q.first], cnt = s.level_off[q.first + 1] - beg;
      KK_LAUNCH((sptrsv_level_kernel<OffT, VT>), (unsigned)ceil_div(cnt * q.lpr, kBlock), kBlock, 0, st, (const int32_t*)(s.d_grouped + beg), cnt, q.lpr,
                sh, rm, ent, val, (const int32_t*)h->d_diagpos, b, x);
    }
  }
  KK_LAUNCH_CHECK();
  return KKAMD_OK;
}

}  // namespace kk

extern "C" {

int kkamd_sptrsv_create(kkamd_sptrsv_handle_t** handle, int algorithm, int64_t num_rows, int lower_tri) {
  if (!handle) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_create: null handle pointer");
  *handle = nullptr;
  if (algorithm == KKAMD_SPTRSV_CUSPARSE)
    return kk::fail(KKAMD_ERR_UNSUPPORTED, "kkamd_sptrsv_create: SPTRSV_CUSPARSE is not available here (use a SEQLVLSCHD algorithm)");
  if (algorithm < KKAMD_SPTRSV_SEQLVLSCHD_RP || algorithm > KKAMD_SPTRSV_CUSPARSE)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_create: unknown SPTRSVAlgorithm %d", algorithm);
  if (num_rows < 0 || num_rows > (int64_t)INT32_MAX)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_create: num_rows %lld is outside [0, 2^31)", (long long)num_rows);
  kkamd_sptrsv_handle* h = new (std::nothrow) kkamd_sptrsv_handle();
  if (!h) return kk::fail(KKAMD_ERR_ALLOC, "kkamd_sptrsv_create: out of host memory");
  h->algorithm = algorithm;
  h->nrows     = num_rows;
  h->lower     = lower_tri ? 1 : 0;
  *handle      = h;
  return KKAMD_OK;
}

int kkamd_sptrsv_destroy(kkamd_sptrsv_handle_t* h) {
  if (!h) return KKAMD_OK;
  h->clear_symbolic();
  delete h;
  return KKAMD_OK;
}

int kkamd_sptrsv_symbolic(kkamd_sptrsv_handle_t* h, int64_t num_rows, const void* d_row_map, const int32_t* d_entries, int offset_type,
                          kkamd_stream_t stream) {
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_symbolic: null handle");
  if (num_rows != h->nrows)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_symbolic: num_rows %lld differs from the handle's %lld", (long long)num_rows, (long long)h->nrows);
  if (offset_type != KKAMD_I32 && offset_type != KKAMD_I64) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_symbolic: unknown offset_type %d", offset_type);
  if (num_rows > 0 && (!d_row_map || !d_entries)) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_symbolic: null pointer");
  kk::TraceRange range("KokkosSparse::sptrsv_symbolic[TPL_KKAMD]");
  hipStream_t st = kk::to_hip(stream);
  h->clear_symbolic();                                       // a repeated call analyses again
  kk::DevBuf level_list, diagpos;
  const int rc = kk::analyse_levels(&h->sched, num_rows, h->lower, d_row_map, d_entries, offset_type, st, &level_list, &diagpos);
  if (rc) return rc;
  h->d_level_list = (int32_t*)level_list.release();
  h->d_diagpos    = (int32_t*)diagpos.release();
  kk::sptrsv_build_plan(h);
  h->symbolic_complete = true;
  return KKAMD_OK;
}

int kkamd_sptrsv_solve(kkamd_sptrsv_handle_t* h, int64_t num_rows, const void* d_row_map, const int32_t* d_entries, const void* d_values,
                       const void* d_b, void* d_x, int offset_type, int value_type, kkamd_stream_t stream) {
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_solve: null handle");
  if (!h->symbolic_complete) return kk::fail(KKAMD_ERR_STATE, "KokkosSparse::sptrsv_solve: the symbolic phase has not been completed on this handle");
  if (value_type != KKAMD_F64 && value_type != KKAMD_F32)
    return kk::fail(KKAMD_ERR_UNSUPPORTED, "kkamd_sptrsv_solve: unsupported type pair (value_type %d): (F64,F64) and (F32,F32) are", value_type);
  if (num_rows != h->nrows)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_solve: num_rows %lld differs from the handle's %lld", (long long)num_rows, (long long)h->nrows);
  if (offset_type != KKAMD_I32 && offset_type != KKAMD_I64) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_solve: unknown offset_type %d", offset_type);
  if (num_rows == 0) return KKAMD_OK;
  if (!d_row_map || !d_entries || !d_values || !d_b || !d_x) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_solve: null pointer");
  kk::TraceRange range(value_type == KKAMD_F64 ? "KokkosSparse::sptrsv_solve[TPL_KKAMD,double]" : "KokkosSparse::sptrsv_solve[TPL_KKAMD,float]");
  hipStream_t st = kk::to_hip(stream);
  if (offset_type == KKAMD_I64) {
    if (value_type == KKAMD_F64) return kk::sptrsv_solve_typed<int64_t, double>(h, (const int64_t*)d_row_map, d_entries, (const double*)d_values, (const double*)d_b, (double*)d_x, st);
    return kk::sptrsv_solve_typed<int64_t, float>(h, (const int64_t*)d_row_map, d_entries, (const float*)d_values, (const float*)d_b, (float*)d_x, st);
  }
  if (value_type == KKAMD_F64) return kk::sptrsv_solve_typed<int32_t, double>(h, (const int32_t*)d_row_map, d_entries, (const double*)d_values, (const double*)d_b, (double*)d_x, st);
  return kk::sptrsv_solve_typed<int32_t, float>(h, (const int32_t*)d_row_map, d_entries, (const float*)d_values, (const float*)d_b, (float*)d_x, st);
}

int kkamd_sptrsv_set(kkamd_sptrsv_handle_t* h, const char* key, int value) {
  if (!h || !key) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_set: null argument");
  const int rc = kk::set_knob(&h->sched, "kkamd_sptrsv_set", key, value);
  if (rc) return rc;
  if (h->symbolic_complete) kk::sptrsv_build_plan(h);
  return KKAMD_OK;
}

int kkamd_sptrsv_get(const kkamd_sptrsv_handle_t* h, const char* key, int64_t* value) {
  if (!h || !key || !value) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_get: null argument");
  const std::string k(key);
  if (kk::get_common(h->sched, k, value)) return KKAMD_OK;
  if (k == "symbolic_complete") *value = h->symbolic_complete ? 1 : 0;
  else if (k == "lower_tri") *value = h->lower;
  else if (k == "algorithm") *value = h->algorithm;
  else if (k == "num_rows") *value = h->nrows;
  else if (k == "plan_bytes")
    *value = h->d_level_list ? (int64_t)(3 * sizeof(int32_t)) * h->nrows + (int64_t)sizeof(int64_t) * (h->sched.num_levels() + 1) : 0;
  else return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_get: unknown key '%s'", key);
  return KKAMD_OK;
}

int kkamd_sptrsv_export(const kkamd_sptrsv_handle_t* h, const char* what, void* h_out, int64_t count) {
  if (!h || !what) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_export: null argument");
  if (!h->symbolic_complete) return kk::fail(KKAMD_ERR_STATE, "kkamd_sptrsv_export: the symbolic phase has not been completed on this handle");
  const std::string k(what);
  const bool per_level = k == "nodes_per_level";
  if (!per_level && k != "level_list" && k != "nodes_grouped_by_level") return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_export: unknown array '%s'", what);
  const int64_t need = per_level ? h->sched.num_levels() : h->nrows;
  if (count != need) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_export: '%s' has %lld entries, not %lld", what, (long long)need, (long long)count);
  if (need == 0) return KKAMD_OK;
  if (!h_out) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_sptrsv_export: null output");
  int32_t* out = (int32_t*)h_out;
  if (per_level) {
    for (int64_t l = 0; l < need; ++l) out[l] = (int32_t)(h->sched.level_off[l + 1] - h->sched.level_off[l]);
    return KKAMD_OK;
  }
  KK_HIP(hipMemcpy(out, k == "level_list" ? h->d_level_list : h->sched.d_grouped, sizeof(int32_t) * (size_t)need, hipMemcpyDeviceToHost));
  return KKAMD_OK;
}

}  // extern "C"
