// kk_spiluk.hip -- level-scheduled incomplete LU factorisation with level of fill k: KokkosSparse::spiluk_symbolic / spiluk_numeric
// (sparse/src/KokkosSparse_spiluk.hpp, handle sparse/src/KokkosSparse_spiluk_handle.hpp) for a square CrsMatrix.
//
// Symbolic phase (sparse/impl/KokkosSparse_spiluk_symbolic_impl.hpp:212-418).  As in the reference the fill computation runs on the
// host: the graph of A is copied down, validated before anything is indexed by it, run through the reference's sum-rule loop
// (kk_spiluk_fill.h) and the graphs of L and U are copied up.  It runs once per pattern.  The level sets are those of L (:400-402):
// level(i) = 1 + max level(col) over the off-diagonal columns of L row i, rows ascending inside a level.  That is what the analysis
// of the triangular solve computes on the device (kk_sptrsv.hip): it runs on L, and the handle keeps the schedule it fills.
//
// Numeric phase (sparse/impl/KokkosSparse_spiluk_numeric_impl.hpp:438-551, level loop :572-617).  One launch per level; a group of
// LPR lanes owns one row i:
//   L(i,:) = 0, L(i,i) = 1, U(i,:) = 0; row i of A is scattered into them;
//   for every off-diagonal column k of L row i, ascending: L(i,k) /= U(k,k), and every off-diagonal (k,c) of U row k that row i's
//   pattern holds gets X(i,c) = X(i,c) - L(i,k) * U(k,c), X = L for c < i, U otherwise;
//   U(i,i) == 0 becomes 1e6 (:528-534).
// Every entry takes its updates one pivot at a time in ascending k and each update touches one entry once, so the values do not
// depend on the lane mapping: the same bits on every run and under every knob.  The reference finds (i,c) through a dense
// level_maxrows x nrows position array (spiluk_handle.hpp:178-181); here column c is found by bisection of the sorted row, its L part
// for c < i, its U part otherwise.  A row whose L and U parts together fit kStage entries per lane is staged in LDS (columns and
// working values) and written back once; a longer row works on L_values / U_values in global memory.
// Runs of consecutive narrow levels are chained into one single-workgroup launch with __syncthreads() between the levels.
// No work-item ever waits on another workgroup: every dependency between workgroups is a kernel boundary on the stream.
//
// Not here: the block (BSR) variant, spiluk_numeric_streams, a device-side fill computation, the reference-side TPL binding.
#include "kk_levels.h"
#include "kk_spiluk_fill.h"
#include <chrono>
#include <climits>
#include <cstring>
#include <new>

// Orders one lane group's memory operations between two steps of a row: what a lane stored before it (LDS or global memory) is
// visible to the loads of the other lanes after it.  Release and acquire fences at workgroup scope around the wave barrier; nothing
// relies on the lanes of a wavefront running in lock step.
#ifdef KK_EMU
#define KK_GROUP_SYNC() kk_emu::sync_wave()
#else
#define KK_GROUP_SYNC()                                     \
  do {                                                      \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  \
    __builtin_amdgcn_wave_barrier();                        \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");  \
  } while (0)
#endif

namespace kk {

constexpr int kStage = 4;   // LDS entries per lane: a group of LPR lanes stages rows of up to kStage * LPR entries (L and U parts together)

// position of column c in the ascending list col[0 .. len), -1 when it is not there
__device__ __forceinline__ int find_col(const int32_t* col, int len, int32_t c) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (col[mid] < c) lo = mid + 1; else hi = mid;
  }
  return (lo < len && col[lo] == c) ? lo : -1;
}

// One row per group of lpr lanes (a power of two, 1..64).  Every lane of the wavefront goes through every KK_GROUP_SYNC and shuffle
// the same number of times (the pivot loop runs to the wavefront's longest L row), lanes without a row included.
// L_val and U_val: rows of earlier levels were written by an earlier launch, or by this workgroup before its last barrier; they are
// neither const nor __restrict__, so they are read with ordinary vector loads.
template <class OffT, class VT>
__device__ __forceinline__ void spiluk_row(bool valid, int32_t row, int lane, int lpr, int32_t* sc, VT* sv, const OffT* __restrict__ A_rm,
                                           const int32_t* __restrict__ A_ent, const VT* __restrict__ A_val, const OffT* __restrict__ L_rm,
                                           const int32_t* __restrict__ L_ent, VT* L_val, const OffT* __restrict__ U_rm,
                                           const int32_t* __restrict__ U_ent, VT* U_val) {
  int64_t ls = 0, us = 0;
  int nl = 0, nu = 0;                                        // nl counts the unit diagonal at the end of the L row
  if (valid) {
    ls = (int64_t)L_rm[row]; nl = (int)((int64_t)L_rm[row + 1] - ls);
    us = (int64_t)U_rm[row]; nu = (int)((int64_t)U_rm[row + 1] - us);
  }
  const bool staged = valid && nl + nu <= kStage * lpr;
  const int32_t *lc = L_ent + ls, *uc = U_ent + us;
  VT *lv = L_val + ls, *uv = U_val + us;
  if (staged) {
    for (int j = lane; j < nl + nu; j += lpr) {
      sc[j] = j < nl ? L_ent[ls + j] : U_ent[us + (j - nl)];
      sv[j] = j == nl - 1 ? VT(1) : VT(0);
    }
    lc = sc; uc = sc + nl; lv = sv; uv = sv + nl;
  } else if (valid) {
    for (int j = lane; j < nl; j += lpr) lv[j] = j == nl - 1 ? VT(1) : VT(0);
    for (int j = lane; j < nu; j += lpr) uv[j] = VT(0);
  }
  KK_GROUP_SYNC();
  const int np = nl > 0 ? nl - 1 : 0;                        // pivots: the off-diagonal columns of the L row
  if (valid) {
    const int64_t ae = (int64_t)A_rm[row + 1];
    for (int64_t p = (int64_t)A_rm[row] + lane; p < ae; p += lpr) {
      const int32_t c = A_ent[p];
      const int pos = c < row ? find_col(lc, np, c) : find_col(uc, nu, c);
      if (pos >= 0) (c < row ? lv : uv)[pos] = A_val[p];
    }
  }
  int maxp = np;
  for (int o = kWave >> 1; o > 0; o >>= 1) { const int t = __shfl_xor(maxp, o, 64); maxp = t > maxp ? t : maxp; }
  for (int kk = 0; kk < maxp; ++kk) {
    KK_GROUP_SYNC();                                         // the updates of the pivot before are visible
    const bool act = kk < np;
    VT f = VT(0);
    int32_t k = 0;
    if (act && lane == 0) {
      k = lc[kk];
      f = lv[kk] / U_val[(int64_t)U_rm[k]];                 // the diagonal is first in a row of U
      lv[kk] = f;                                            // no update of this or a later pivot touches column k again
    }
    f = __shfl(f, 0, lpr);
    k = __shfl(k, 0, lpr);
    if (act) {
      const int64_t ue = (int64_t)U_rm[k + 1];
      for (int64_t p = (int64_t)U_rm[k] + 1 + lane; p < ue; p += lpr) {
        const int32_t c = U_ent[p];
        const int pos = c < row ? find_col(lc, np, c) : find_col(uc, nu, c);
        if (pos >= 0) {
          VT* x = (c < row ? lv : uv) + pos;
          *x = *x - f * U_val[p];
        }
      }
    }
  }
  KK_GROUP_SYNC();
  if (valid && lane == 0 && nu > 0 && uv[0] == VT(0)) uv[0] = VT(1e6);
  KK_GROUP_SYNC();
  if (staged)
    for (int j = lane; j < nl + nu; j += lpr) {
      if (j < nl) L_val[ls + j] = sv[j]; else U_val[us + (j - nl)] = sv[j];
    }
  KK_GROUP_SYNC();                                           // the group's LDS slice is free for its next row
}

template <class OffT, class VT>
__global__ __launch_bounds__(kBlock) void spiluk_level_kernel(const int32_t* __restrict__ rows, int64_t cnt, int lpr, int lpr_shift,
                                                              const OffT* __restrict__ A_rm, const int32_t* __restrict__ A_ent,
                                                              const VT* __restrict__ A_val, const OffT* __restrict__ L_rm,
                                                              const int32_t* __restrict__ L_ent, VT* L_val, const OffT* __restrict__ U_rm,
                                                              const int32_t* __restrict__ U_ent, VT* U_val) {
  __shared__ int32_t s_col[kBlock * kStage];
  __shared__ VT s_val[kBlock * kStage];
  const int64_t g = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> lpr_shift;
  const int slice = ((int)threadIdx.x >> lpr_shift) * lpr * kStage;
  const bool valid = g < cnt;
  spiluk_row<OffT, VT>(valid, valid ? rows[g] : 0, threadIdx.x & (lpr - 1), lpr, s_col + slice, s_val + slice, A_rm, A_ent, A_val, L_rm, L_ent,
                       L_val, U_rm, U_ent, U_val);
}

// levels [first, first + nlev) in one workgroup; the barrier's workgroup-scope ordering is all L_val / U_val need between them
template <class OffT, class VT>
__global__ __launch_bounds__(kBlock) void spiluk_chain_kernel(const int32_t* __restrict__ grouped, const int64_t* __restrict__ level_off, int first,
                                                              int nlev, int lpr, int lpr_shift, const OffT* __restrict__ A_rm,
                                                              const int32_t* __restrict__ A_ent, const VT* __restrict__ A_val,
                                                              const OffT* __restrict__ L_rm, const int32_t* __restrict__ L_ent, VT* L_val,
                                                              const OffT* __restrict__ U_rm, const int32_t* __restrict__ U_ent, VT* U_val) {
  __shared__ int32_t s_col[kBlock * kStage];
  __shared__ VT s_val[kBlock * kStage];
  const int lane = threadIdx.x & (lpr - 1), grp = threadIdx.x >> lpr_shift, ngrp = kBlock >> lpr_shift;
  const int slice = grp * lpr * kStage;
  for (int l = first; l < first + nlev; ++l) {
    const int64_t beg = level_off[l], cnt = level_off[l + 1] - beg;
    for (int64_t base = 0; base < cnt; base += ngrp) {       // uniform trip count: every lane reaches every rendezvous
      const bool valid = base + grp < cnt;
      spiluk_row<OffT, VT>(valid, valid ? grouped[beg + base + grp] : 0, lane, lpr, s_col + slice, s_val + slice, A_rm, A_ent, A_val, L_rm,
                           L_ent, L_val, U_rm, U_ent, U_val);
    }
    __syncthreads();
  }
}

}  // namespace kk

struct kkamd_spiluk_handle {
  int algorithm = 0;
  int64_t nrows = 0, nnzL = 0, nnzU = 0;
  bool symbolic_complete = false;
  kk::LevelSchedule sched;                                 // of L
  std::vector<int32_t> level_list, level_ptr, level_idx;  // host, as the reference's handle holds them (level_list 1-based)
  int64_t fill_us = 0, levels_us = 0;                      // host fill loop; everything else of the last symbolic call

  void clear_symbolic() {
    symbolic_complete = false;
    sched.clear();
    level_list.clear(); level_ptr.clear(); level_idx.clear();
  }
};

namespace kk {

// one lane count for every launch: what covers the mean row of U
static int spiluk_lanes(const kkamd_spiluk_handle* h) {
  return h->sched.lanes_per_row ? h->sched.lanes_per_row : pow2_covering(h->nrows > 0 ? ceil_div(h->nnzU, h->nrows) : 1);
}

// the launches of one numeric call; every set builds them again, so the lane count stored with each stays right
static void spiluk_build_plan(kkamd_spiluk_handle* h) {
  const int lpr = spiluk_lanes(h);
  build_plan(&h->sched, h->sched.chain_rows > 0, [lpr](int64_t, int64_t) { return lpr; });
}

template <class OffT>
static int spiluk_symbolic_typed(kkamd_spiluk_handle* h, int fill_lev, int64_t n, const OffT* A_rm, const int32_t* A_ent, OffT* L_rm,
                                 int32_t* L_ent, int64_t L_cap, OffT* U_rm, int32_t* U_ent, int64_t U_cap, int offset_type, hipStream_t st) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  std::vector<OffT> rm((size_t)n + 1);
  KK_HIP(hipMemcpyAsync(rm.data(), A_rm, sizeof(OffT) * (size_t)(n + 1), hipMemcpyDeviceToHost, st));
  KK_HIP(hipStreamSynchronize(st));
  int64_t bad = -1;
  if (iluk_check_row_map<OffT>(n, rm.data(), &bad))
    return fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_symbolic: row %lld: A's row_map offsets are not ascending", (long long)bad);
  const int64_t a0 = (int64_t)rm[0], nnz = (int64_t)rm[(size_t)n] - a0;
  std::vector<int32_t> ent((size_t)nnz);
  if (nnz > 0) {
    KK_HIP(hipMemcpyAsync(ent.data(), A_ent + a0, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, st));
    KK_HIP(hipStreamSynchronize(st));
  }
  if (a0)
    for (OffT& r : rm) r = (OffT)((int64_t)r - a0);          // ent holds the entries from A_rm[0] on
  if (const int kind = iluk_check_entries<OffT>(n, rm.data(), ent.data(), &bad))
    return fail(KKAMD_ERR_INVALID_ARG, kind == kFillColumn ? "kkamd_spiluk_symbolic: row %lld: a column of A is outside [0, num_rows)"
                                                           : "kkamd_spiluk_symbolic: row %lld: a column of A is repeated", (long long)bad);
  const auto t1 = clock::now();
  IlukPattern pat;
  iluk_fill<OffT>(n, rm.data(), ent.data(), fill_lev, &pat);
  const auto t2 = clock::now();
  const int64_t nnzL = (int64_t)pat.L_ent.size(), nnzU = (int64_t)pat.U_ent.size();
  // the reference's texts (symbolic_impl.hpp:353-357,375-379), with the whole of L and U counted
  if (nnzU > U_cap)
    return fail(KKAMD_ERR_INVALID_ARG, "KokkosSparse::Experimental::spiluk_symbolic: U_entries's extent must be larger than %lld, must be at least %lld",
                (long long)U_cap, (long long)nnzU);
  if (nnzL > L_cap)
    return fail(KKAMD_ERR_INVALID_ARG, "KokkosSparse::Experimental::spiluk_symbolic: L_entries's extent must be larger than %lld, must be at least %lld",
                (long long)L_cap, (long long)nnzL);
  if (offset_type == KKAMD_I32 && (nnzL > (int64_t)INT32_MAX || nnzU > (int64_t)INT32_MAX))
    return fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_symbolic: L or U has more than 2^31 - 1 entries: use 64-bit offsets");
  std::vector<OffT> lrm((size_t)n + 1), urm((size_t)n + 1);
  for (int64_t i = 0; i <= n; ++i) { lrm[(size_t)i] = (OffT)pat.L_rm[(size_t)i]; urm[(size_t)i] = (OffT)pat.U_rm[(size_t)i]; }
  KK_HIP(hipMemcpyAsync(L_rm, lrm.data(), sizeof(OffT) * (size_t)(n + 1), hipMemcpyHostToDevice, st));
  KK_HIP(hipMemcpyAsync(U_rm, urm.data(), sizeof(OffT) * (size_t)(n + 1), hipMemcpyHostToDevice, st));
  if (nnzL > 0) KK_HIP(hipMemcpyAsync(L_ent, pat.L_ent.data(), sizeof(int32_t) * (size_t)nnzL, hipMemcpyHostToDevice, st));
  if (nnzU > 0) KK_HIP(hipMemcpyAsync(U_ent, pat.U_ent.data(), sizeof(int32_t) * (size_t)nnzU, hipMemcpyHostToDevice, st));
  KK_HIP(hipStreamSynchronize(st));                          // the host vectors go out of use
  // the level sets of L: the schedule stays as the analysis leaves it; level_list and the diagonal positions are not kept on the device
  DevBuf list_b, diag_b;
  {
    TraceRange levels("KokkosSparse::sptrsv_symbolic[TPL_KKAMD]");
    const int rc = analyse_levels(&h->sched, n, 1, L_rm, L_ent, offset_type, st, &list_b, &diag_b);
    if (rc) return rc;
  }
  h->level_list.assign((size_t)n, 0);
  h->level_idx.assign((size_t)n, 0);
  if (n > 0) {
    KK_HIP(hipMemcpyAsync(h->level_list.data(), list_b.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    KK_HIP(hipMemcpyAsync(h->level_idx.data(), h->sched.d_grouped, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    KK_HIP(hipStreamSynchronize(st));
  }
  h->level_ptr.assign(h->sched.level_off.begin(), h->sched.level_off.end());   // offsets up to n < 2^31
  h->nnzL = nnzL;
  h->nnzU = nnzU;
  const auto t3 = clock::now();
  h->fill_us   = (int64_t)std::chrono::duration_cast<std::chrono::microseconds>(t2 - t1).count();
  h->levels_us = (int64_t)std::chrono::duration_cast<std::chrono::microseconds>((t1 - t0) + (t3 - t2)).count();
  return KKAMD_OK;
}

template <class OffT, class VT>
static int spiluk_numeric_typed(const kkamd_spiluk_handle* h, const OffT* A_rm, const int32_t* A_ent, const VT* A_val, const OffT* L_rm,
                                const int32_t* L_ent, VT* L_val, const OffT* U_rm, const int32_t* U_ent, VT* U_val, hipStream_t st) {
  const LevelSchedule& s = h->sched;
  for (const LevelLaunch& q : s.plan) {
    const int sh = log2i(q.lpr);
    if (q.chain) {
      KK_LAUNCH((spiluk_chain_kernel<OffT, VT>), 1u, kBlock, 0, st, (const int32_t*)s.d_grouped, (const int64_t*)s.d_level_off, q.first, q.nlev, q.lpr, sh,
                A_rm, A_ent, A_val, L_rm, L_ent, L_val, U_rm, U_ent, U_val);
    } else {
      const int64_t beg = s.level_off[q.first], cnt = s.level_off[q.first + 1] - beg;
      KK_LAUNCH((spiluk_level_kernel<OffT, VT>), (unsigned)ceil_div(cnt * q.lpr, kBlock), kBlock, 0, st, (const int32_t*)(s.d_grouped + beg), cnt, q.lpr, sh,
                A_rm, A_ent, A_val, L_rm, L_ent, L_val, U_rm, U_ent, U_val);
    }
  }
  KK_LAUNCH_CHECK();
  return KKAMD_OK;
}

}  // namespace kk

extern "C" {

int kkamd_spiluk_create(kkamd_spiluk_handle_t** handle, int algorithm, int64_t num_rows, int64_t nnzL, int64_t nnzU) {
  if (!handle) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_create: null handle pointer");
  *handle = nullptr;
  if (algorithm != KKAMD_SPILUK_SEQLVLSCHD_TP1) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_create: unknown SPILUKAlgorithm %d", algorithm);
  if (num_rows < 0 || num_rows > (int64_t)INT32_MAX)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_create: num_rows %lld is outside [0, 2^31)", (long long)num_rows);
  if (nnzL < 0 || nnzU < 0) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_create: negative nnzL or nnzU");
  kkamd_spiluk_handle* h = new (std::nothrow) kkamd_spiluk_handle();
  if (!h) return kk::fail(KKAMD_ERR_ALLOC, "kkamd_spiluk_create: out of host memory");
  h->algorithm = algorithm;
  h->nrows     = num_rows;
  h->nnzL      = nnzL;
  h->nnzU      = nnzU;
  *handle      = h;
  return KKAMD_OK;
}

int kkamd_spiluk_destroy(kkamd_spiluk_handle_t* h) {
  if (!h) return KKAMD_OK;
  h->sched.clear();
  delete h;
  return KKAMD_OK;
}

int kkamd_spiluk_symbolic(kkamd_spiluk_handle_t* h, int fill_lev, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries,
                          void* d_L_row_map, int32_t* d_L_entries, int64_t L_capacity, void* d_U_row_map, int32_t* d_U_entries, int64_t U_capacity,
                          int offset_type, kkamd_stream_t stream) {
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_symbolic: null handle");
  if (fill_lev < 0)   // the reference's text (sparse/src/KokkosSparse_spiluk.hpp)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "KokkosSparse::Experimental::spiluk_symbolic: fill_lev: %d. Valid value is >= 0.", fill_lev);
  if (num_rows != h->nrows)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_symbolic: num_rows %lld differs from the handle's %lld", (long long)num_rows, (long long)h->nrows);
  if (offset_type != KKAMD_I32 && offset_type != KKAMD_I64) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_symbolic: unknown offset_type %d", offset_type);
  if (L_capacity < 0 || U_capacity < 0) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_symbolic: negative capacity");
  if (!d_A_row_map || !d_L_row_map || !d_U_row_map) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_symbolic: null row_map");
  if (num_rows > 0 && (!d_L_entries || !d_U_entries)) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_symbolic: null pointer");
  kk::TraceRange range("KokkosSparse::spiluk_symbolic[TPL_KKAMD]");
  hipStream_t st = kk::to_hip(stream);
  h->clear_symbolic();                                       // a repeated call analyses again
  const int rc = offset_type == KKAMD_I64
                     ? kk::spiluk_symbolic_typed<int64_t>(h, fill_lev, num_rows, (const int64_t*)d_A_row_map, d_A_entries, (int64_t*)d_L_row_map, d_L_entries,
                                                          L_capacity, (int64_t*)d_U_row_map, d_U_entries, U_capacity, offset_type, st)
                     : kk::spiluk_symbolic_typed<int32_t>(h, fill_lev, num_rows, (const int32_t*)d_A_row_map, d_A_entries, (int32_t*)d_L_row_map, d_L_entries,
                                                          L_capacity, (int32_t*)d_U_row_map, d_U_entries, U_capacity, offset_type, st);
  if (rc) { h->clear_symbolic(); return rc; }
  kk::spiluk_build_plan(h);
  h->symbolic_complete = true;
  return KKAMD_OK;
}

int kkamd_spiluk_numeric(kkamd_spiluk_handle_t* h, int fill_lev, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries,
                         const void* d_A_values, const void* d_L_row_map, const int32_t* d_L_entries, void* d_L_values, const void* d_U_row_map,
                         const int32_t* d_U_entries, void* d_U_values, int offset_type, int value_type, kkamd_stream_t stream) {
  (void)fill_lev;   // as in the reference, the pattern of L and U carries it
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_numeric: null handle");
  if (!h->symbolic_complete) return kk::fail(KKAMD_ERR_STATE, "KokkosSparse::spiluk_numeric: the symbolic phase has not been completed on this handle");
  if (value_type != KKAMD_F64 && value_type != KKAMD_F32)
    return kk::fail(KKAMD_ERR_UNSUPPORTED, "kkamd_spiluk_numeric: unsupported value_type %d: F64 and F32 are", value_type);
  if (num_rows != h->nrows)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_numeric: num_rows %lld differs from the handle's %lld", (long long)num_rows, (long long)h->nrows);
  if (offset_type != KKAMD_I32 && offset_type != KKAMD_I64) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_numeric: unknown offset_type %d", offset_type);
  if (num_rows == 0) return KKAMD_OK;
  if (!d_A_row_map || !d_L_row_map || !d_L_entries || !d_L_values || !d_U_row_map || !d_U_entries || !d_U_values)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_numeric: null pointer");
  kk::TraceRange range(value_type == KKAMD_F64 ? "KokkosSparse::spiluk_numeric[TPL_KKAMD,double]" : "KokkosSparse::spiluk_numeric[TPL_KKAMD,float]");
  hipStream_t st = kk::to_hip(stream);
  if (offset_type == KKAMD_I64) {
    if (value_type == KKAMD_F64)
      return kk::spiluk_numeric_typed<int64_t, double>(h, (const int64_t*)d_A_row_map, d_A_entries, (const double*)d_A_values, (const int64_t*)d_L_row_map,
                                                       d_L_entries, (double*)d_L_values, (const int64_t*)d_U_row_map, d_U_entries, (double*)d_U_values, st);
    return kk::spiluk_numeric_typed<int64_t, float>(h, (const int64_t*)d_A_row_map, d_A_entries, (const float*)d_A_values, (const int64_t*)d_L_row_map,
                                                    d_L_entries, (float*)d_L_values, (const int64_t*)d_U_row_map, d_U_entries, (float*)d_U_values, st);
  }
  if (value_type == KKAMD_F64)
    return kk::spiluk_numeric_typed<int32_t, double>(h, (const int32_t*)d_A_row_map, d_A_entries, (const double*)d_A_values, (const int32_t*)d_L_row_map,
                                                     d_L_entries, (double*)d_L_values, (const int32_t*)d_U_row_map, d_U_entries, (double*)d_U_values, st);
  return kk::spiluk_numeric_typed<int32_t, float>(h, (const int32_t*)d_A_row_map, d_A_entries, (const float*)d_A_values, (const int32_t*)d_L_row_map,
                                                  d_L_entries, (float*)d_L_values, (const int32_t*)d_U_row_map, d_U_entries, (float*)d_U_values, st);
}

int kkamd_spiluk_set(kkamd_spiluk_handle_t* h, const char* key, int value) {
  if (!h || !key) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_set: null argument");
  const int rc = kk::set_knob(&h->sched, "kkamd_spiluk_set", key, value);
  if (rc) return rc;
  if (h->symbolic_complete) kk::spiluk_build_plan(h);
  return KKAMD_OK;
}

int kkamd_spiluk_get(const kkamd_spiluk_handle_t* h, const char* key, int64_t* value) {
  if (!h || !key || !value) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_get: null argument");
  const std::string k(key);
  if (kk::get_common(h->sched, k, value)) return KKAMD_OK;
  if (k == "nnzL") *value = h->nnzL;
  else if (k == "nnzU") *value = h->nnzU;
  else if (k == "symbolic_complete") *value = h->symbolic_complete ? 1 : 0;
  else if (k == "algorithm") *value = h->algorithm;
  else if (k == "num_rows") *value = h->nrows;
  else if (k == "lanes_in_use") *value = kk::spiluk_lanes(h);
  else if (k == "stage_entries_per_lane") *value = kk::kStage;
  else if (k == "symbolic_fill_us") *value = h->fill_us;
  else if (k == "symbolic_other_us") *value = h->levels_us;
  else if (k == "plan_bytes")   // the rows grouped by level and the level offsets; an empty matrix counts its one offset, as it always has
    *value = h->symbolic_complete ? (int64_t)sizeof(int32_t) * h->nrows + (int64_t)sizeof(int64_t) * (h->sched.num_levels() + 1) : 0;
  else return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_get: unknown key '%s'", key);
  return KKAMD_OK;
}

int kkamd_spiluk_export(const kkamd_spiluk_handle_t* h, const char* what, void* h_out, int64_t count) {
  if (!h || !what) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_export: null argument");
  if (!h->symbolic_complete) return kk::fail(KKAMD_ERR_STATE, "kkamd_spiluk_export: the symbolic phase has not been completed on this handle");
  const std::string k(what);
  const std::vector<int32_t>* src = k == "level_list" ? &h->level_list : k == "level_ptr" ? &h->level_ptr : k == "level_idx" ? &h->level_idx : nullptr;
  if (!src) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_export: unknown array '%s'", what);
  const int64_t need = (int64_t)src->size();
  if (count != need) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_export: '%s' has %lld entries, not %lld", what, (long long)need, (long long)count);
  if (need == 0) return KKAMD_OK;
  if (!h_out) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_spiluk_export: null output");
  std::memcpy(h_out, src->data(), sizeof(int32_t) * (size_t)need);
  return KKAMD_OK;
}

}  // extern "C"
