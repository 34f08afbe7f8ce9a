// kk_gmres.hip -- restarted GMRES with right preconditioning: KokkosSparse::Experimental::gmres (sparse/src/KokkosSparse_gmres.hpp; the
// loop is sparse/impl/KokkosSparse_gmres_impl.hpp:59-329, the handle sparse/src/KokkosSparse_gmres_handle.hpp), the preconditioner
// interface with MatrixPrec and LUPrec (sparse/src/KokkosSparse_Preconditioner.hpp, KokkosSparse_MatrixPrec.hpp, KokkosSparse_LUPrec.hpp),
// and the orthogonalisation kernels on the tall-skinny basis V (n x (m + 1), column-major, column stride ldv >= n).
//
// Every reduction has one fixed order.  The rows are cut into G = ceil(n / R) groups of R rows, R a function of n and the knob
// "rows_per_group" alone (gm_rows_per_group).  Group g is one workgroup of 256 lanes; lane t owns the rows g R + t, g R + t + 256, ... and
// adds their terms in ascending order; the 256 lane sums are added by a xor-shuffle tree inside each wave and the four wave sums in
// wave order (gm_block_reduce); the group's sum goes to P[g * k + c] by a plain store; the consumer -- the prologue of the next kernel,
// in every workgroup -- adds the G partials in ascending g (gm_prologue).  No floating-point atomic, no work-item waits on another
// workgroup: every dependency between workgroups is a kernel boundary on the stream.
//
//   gm_dot_kernel        P[g][c] = partial of V(:,c)^T w; the columns go in register batches of 8, so w is read once per batch and V once
//   gm_update_kernel     prologue h = sum_g Pin[g][:] (workgroup 0 stores h, and hsum = hadd + h when asked); then for its rows
//                        w_out = w_in + alpha * (sum_c V(r,c) h(c)), c ascending, optionally with the partial of sum w_out^2
//   gm_fused_kernel      the same update, and from the same V(r,c) -- a row tile of V staged in LDS, so V crosses HBM once for both uses --
//                        the partial P2[g][c] of V(:,c)^T w_out, in the lane order of gm_dot_kernel: the same bits as update-then-dot
//   gm_normalise_kernel  prologue nrm = sqrt(sum_g SS[g]) in the value type (workgroup 0 stores it); then out = w * (1 / nrm), under the
//                        reference's guard nrm > 1e-14 (gmres_impl.hpp:185-188) when asked, taken on the device so the host is not asked
//   gm_axpby_kernel      out = a x + b y with the partial of sum out^2: residuals, norms, and LUPrec's axpby
//
// One CGS2 iteration (gmres_impl.hpp:164-188) is dot, fused update + dot, update + sum of squares, normalise and one device-to-host copy
// of h(0..j) and the norm behind one stream synchronisation: V is read three times instead of the reference's four gemv passes.  The knob
// "fuse" 0, and more columns than the knob "fuse_max_k" (at most kGmFuseMaxK), run dot, update, dot, update + sum of squares: the same
// grouping and lane order, identical bits.
#include "kk_common.h"
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace kk {

constexpr int kGmBatch    = 8;       // columns per register batch of the dot kernel
constexpr int kGmFuseMaxK = 64;      // the fused kernel keeps one accumulator per column and lane
constexpr int kGmFuseDefaultK = 17;  // default of the knob "fuse_max_k": measured on MI355X, the fused kernel wins up to here
constexpr int kGmLdsBytes = 61440;   // LDS a fused workgroup stages its V tile in: with h and the reduction scratch under 64 KB, two workgroups per CU
constexpr int kGmMaxK     = 4096;    // h lives in LDS in the update kernels

// rows per group: the knob when set, else at least 1024 rows and at most about 1024 groups (the prologue of every workgroup reads
// the whole slab: G * k values out of L2)
inline int64_t gm_rows_per_group(int64_t n, int knob) {
  if (knob > 0) return knob;
  const int64_t r = ceil_div(ceil_div(n, 1024), kBlock) * kBlock;
  return r < 1024 ? 1024 : r;
}
inline int64_t gm_groups(int64_t n, int64_t R) { return n > 0 ? ceil_div(n, R) : 1; }
// rows of a fused tile: a power of two that divides the 256 rows of a pass, from k and the LDS budget
inline int gm_tile_rows(int k, size_t value_bytes) {
  int tr = kBlock;
  while (tr > 64 && (size_t)tr * (size_t)k * value_bytes > (size_t)kGmLdsBytes) tr >>= 1;
  return tr;
}

// the sum over the 256 lanes in one fixed order: xor-shuffle tree inside each wave, lane 0 of wave w leaves red[w * stride + c];
// after a barrier gm_block_total adds the four waves in order
template <class T> __device__ __forceinline__ void gm_block_reduce(T v, int c, T* red, int stride) {
  for (int o = kWave >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & (kWave - 1)) == 0) red[(threadIdx.x / kWave) * stride + c] = v;
}
template <class T> __device__ __forceinline__ T gm_block_total(const T* red, int stride, int c) {
  return ((red[c] + red[stride + c]) + red[2 * stride + c]) + red[3 * stride + c];
}

// h[c] = sum over g ascending of Pin[g * k + c], c < k, into LDS; the caller's barrier publishes it
template <class T> __device__ __forceinline__ void gm_prologue(const T* __restrict__ Pin, int64_t gin, int k, T* h) {
  for (int c = threadIdx.x; c < k; c += kBlock) {
    T s = 0;
    for (int64_t g = 0; g < gin; ++g) s += Pin[g * k + c];
    h[c] = s;
  }
}

template <class T>
__global__ __launch_bounds__(kBlock) void gm_dot_kernel(int64_t n, int k, const T* __restrict__ V, int64_t ldv, const T* __restrict__ w,
                                                        int64_t R, T* __restrict__ P) {
  __shared__ T red[4 * kGmBatch];
  const int64_t g = blockIdx.x, r0 = g * R, r1 = (r0 + R < n) ? r0 + R : n;
  for (int cb = 0; cb < k; cb += kGmBatch) {
    T acc[kGmBatch];
    KK_UNROLL
    for (int i = 0; i < kGmBatch; ++i) acc[i] = 0;
    const int nb = (k - cb < kGmBatch) ? k - cb : kGmBatch;
    if (nb == kGmBatch) {
      for (int64_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
        const T wv = w[r];
        KK_UNROLL
        for (int i = 0; i < kGmBatch; ++i) acc[i] += V[(int64_t)(cb + i) * ldv + r] * wv;
      }
    } else {
      for (int64_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
        const T wv = w[r];
        KK_UNROLL
        for (int i = 0; i < kGmBatch; ++i)
          if (i < nb) acc[i] += V[(int64_t)(cb + i) * ldv + r] * wv;
      }
    }
    KK_UNROLL
    for (int i = 0; i < kGmBatch; ++i) gm_block_reduce(acc[i], i, red, kGmBatch);
    __syncthreads();
    if ((int)threadIdx.x < nb) P[g * k + cb + threadIdx.x] = gm_block_total(red, kGmBatch, (int)threadIdx.x);
    __syncthreads();
  }
}

// dynamic LDS: h[k]
template <class T>
__global__ __launch_bounds__(kBlock) void gm_update_kernel(int64_t n, int k, T alpha, const T* __restrict__ V, int64_t ldv,
                                                           const T* __restrict__ Pin, int64_t gin, T* __restrict__ h_out,
                                                           const T* __restrict__ hadd, T* __restrict__ hsum_out, const T* w_in, T* w_out,
                                                           int64_t R, T* __restrict__ SS) {
  KK_DYN_SMEM(T, h);
  __shared__ T red[4];
  gm_prologue(Pin, gin, k, h);
  __syncthreads();
  if (blockIdx.x == 0)
    for (int c = threadIdx.x; c < k; c += kBlock) {
      if (h_out) h_out[c] = h[c];
      if (hsum_out) hsum_out[c] = hadd[c] + h[c];
    }
  const int64_t g = blockIdx.x, r0 = g * R, r1 = (r0 + R < n) ? r0 + R : n;
  T ss = 0;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
    T s = 0;
    KK_UNROLL4
    for (int c = 0; c < k; ++c) s += V[(int64_t)c * ldv + r] * h[c];
    const T wn = w_in ? w_in[r] + alpha * s : alpha * s;
    w_out[r] = wn;
    ss += wn * wn;
  }
  if (SS) {
    gm_block_reduce(ss, 0, red, 1);
    __syncthreads();
    if (threadIdx.x == 0) SS[g] = gm_block_total(red, 1, 0);
  }
}

// NB batches of 8 accumulators per lane (k <= 8 NB); dynamic LDS: h[k], red[4 * k], tile[k * TR]
template <class T, int NB>
__global__ __launch_bounds__(kBlock) void gm_fused_kernel(int64_t n, int k, T alpha, const T* __restrict__ V, int64_t ldv,
                                                          const T* __restrict__ Pin, int64_t gin, T* __restrict__ h_out, const T* w_in,
                                                          T* w_out, int64_t R, int TR, T* __restrict__ P2) {
  KK_DYN_SMEM(T, smem);
  T* h = smem;
  T* red = smem + k;
  T* tile = smem + 5 * (int64_t)k;
  gm_prologue(Pin, gin, k, h);
  __syncthreads();
  if (blockIdx.x == 0 && h_out)
    for (int c = threadIdx.x; c < k; c += kBlock) h_out[c] = h[c];
  const int64_t g = blockIdx.x, r0 = g * R, r1 = (r0 + R < n) ? r0 + R : n;
  const int tid = threadIdx.x;
  const int trs = 31 - __clz(TR);                       // TR is a power of two
  T acc[NB * kGmBatch];
  KK_UNROLL
  for (int c = 0; c < NB * kGmBatch; ++c) acc[c] = 0;
  for (int64_t rb = r0; rb < r1; rb += kBlock) {        // one pass: row rb + t belongs to lane t
    for (int sub = 0; sub < kBlock && rb + sub < r1; sub += TR) {
      const int64_t t0 = rb + sub;
      const int nr = (r1 - t0 < TR) ? (int)(r1 - t0) : TR;
      for (int idx = tid; idx < k * TR; idx += kBlock) {
        const int c = idx >> trs, i = idx & (TR - 1);
        if (i < nr) tile[idx] = V[(int64_t)c * ldv + t0 + i];
      }
      __syncthreads();
      const int i = tid - sub;
      if (i >= 0 && i < nr) {
        const int64_t r = t0 + i;
        T s = 0;
        KK_UNROLL4
        for (int c = 0; c < k; ++c) s += tile[c * TR + i] * h[c];
        const T wn = w_in ? w_in[r] + alpha * s : alpha * s;
        w_out[r] = wn;
        KK_UNROLL
        for (int c = 0; c < NB * kGmBatch; ++c)
          if (c < k) acc[c] += tile[c * TR + i] * wn;
      }
      __syncthreads();
    }
  }
  KK_UNROLL
  for (int c = 0; c < NB * kGmBatch; ++c)
    if (c < k) gm_block_reduce(acc[c], c, red, k);      // k is uniform: every lane of a wave takes the same branch
  __syncthreads();
  if (tid < k) P2[g * k + tid] = gm_block_total(red, k, tid);
}

template <class T>
__global__ __launch_bounds__(kBlock) void gm_normalise_kernel(int64_t n, const T* __restrict__ SS, int64_t gin, T* __restrict__ nrm_out,
                                                              int guard, const T* __restrict__ w, T* __restrict__ out, int64_t R) {
  __shared__ T sh[1];
  if (threadIdx.x == 0) {
    T s = 0;
    for (int64_t g = 0; g < gin; ++g) s += SS[g];
    sh[0] = std::sqrt(s);
    if (blockIdx.x == 0 && nrm_out) *nrm_out = sh[0];
  }
  __syncthreads();
  const T nrm = sh[0];
  if (!out || (guard && !(nrm > 1e-14))) return;
  const T inv = T(1) / nrm;                              // scal(Vj, one / H(j+1,j), Wj)
  const int64_t g = blockIdx.x, r0 = g * R, r1 = (r0 + R < n) ? r0 + R : n;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kBlock) out[r] = inv * w[r];
}

// out = a x + b y (y NULL: a x; out NULL: nothing stored), SS[g] = partial of sum of the squares of what would be stored
template <class T>
__global__ __launch_bounds__(kBlock) void gm_axpby_kernel(int64_t n, T a, const T* x, T b, const T* y, T* out, int64_t R, T* __restrict__ SS) {
  __shared__ T red[4];
  const int64_t g = blockIdx.x, r0 = g * R, r1 = (r0 + R < n) ? r0 + R : n;
  T ss = 0;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += kBlock) {
    const T v = y ? a * x[r] + b * y[r] : a * x[r];
    if (out) out[r] = v;
    ss += v * v;
  }
  if (SS) {
    gm_block_reduce(ss, 0, red, 1);
    __syncthreads();
    if (threadIdx.x == 0) SS[g] = gm_block_total(red, 1, 0);
  }
}

// out[c] = sum_g P[g * k + c] (+ add[c]): the consumer of a slab when no kernel with a prologue follows (the exported building blocks)
template <class T>
__global__ __launch_bounds__(kBlock) void gm_reduce_kernel(const T* __restrict__ P, int64_t gin, int k, T* __restrict__ out) {
  for (int c = threadIdx.x; c < k; c += kBlock) {
    T s = 0;
    for (int64_t g = 0; g < gin; ++g) s += P[g * k + c];
    out[c] = s;
  }
}

}  // namespace kk

using namespace kk;

// ------------------------------------------------------------------------------------------------------------------------------------
// preconditioners
// ------------------------------------------------------------------------------------------------------------------------------------
struct kkamd_precond {
  int kind = 0;                           // 0 matrix, 1 LU, 2 callback
  kkamd_crs_t M{}, L{}, U{};
  kkamd_spmv_plan_t* plan = nullptr;
  kkamd_sptrsv_handle_t* hl = nullptr;
  kkamd_sptrsv_handle_t* hu = nullptr;
  void* d_tmp = nullptr;
  kkamd_precond_fn fn = nullptr;
  void* ctx = nullptr;
};

template <class T>
static int gm_axpby(int64_t n, double a, const void* x, double b, const void* y, void* out, hipStream_t st) {
  if (n == 0) return KKAMD_OK;
  const int64_t R = gm_rows_per_group(n, 0);
  KK_LAUNCH(gm_axpby_kernel<T>, gm_groups(n, R), kBlock, 0, st, n, (T)a, (const T*)x, (T)b, (const T*)y, (T*)out, R, (T*)nullptr);
  KK_LAUNCH_CHECK();
  return KKAMD_OK;
}

extern "C" int kkamd_precond_create_matrix(kkamd_precond_t** p, const kkamd_crs_t* M, kkamd_stream_t stream) {
  if (!p || !M) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_precond_create_matrix: null argument");
  if (int rc = check_crs(M)) return rc;
  kkamd_precond* q = new (std::nothrow) kkamd_precond;
  if (!q) return fail(KKAMD_ERR_ALLOC, "kkamd_precond_create_matrix: out of host memory");
  q->kind = 0; q->M = *M;
  if (int rc = kkamd_spmv_plan_create(&q->plan, M, KKAMD_SPMV_DEFAULT, stream)) { delete q; return rc; }
  *p = q;
  return KKAMD_OK;
}

extern "C" int kkamd_precond_create_lu(kkamd_precond_t** p, const kkamd_crs_t* L, const kkamd_crs_t* U, kkamd_stream_t stream) {
  if (!p || !L || !U) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_precond_create_lu: null argument");
  if (int rc = check_crs(L)) return rc;
  if (int rc = check_crs(U)) return rc;
  if (L->num_rows != U->num_rows) return fail(KKAMD_ERR_INVALID_ARG, "LUPrec: L.numRows() != U.numRows()");
  if (L->value_type != U->value_type || L->offset_type != U->offset_type)
    return fail(KKAMD_ERR_UNSUPPORTED, "kkamd_precond_create_lu: L and U must share their value and offset types");
  kkamd_precond* q = new (std::nothrow) kkamd_precond;
  if (!q) return fail(KKAMD_ERR_ALLOC, "kkamd_precond_create_lu: out of host memory");
  q->kind = 1; q->L = *L; q->U = *U;
  int rc = kkamd_sptrsv_create(&q->hl, KKAMD_SPTRSV_SEQLVLSCHD_TP1, L->num_rows, 1);
  if (!rc) rc = kkamd_sptrsv_create(&q->hu, KKAMD_SPTRSV_SEQLVLSCHD_TP1, U->num_rows, 0);
  // analysed once, here; the reference analyses again at every apply (KokkosSparse_LUPrec.hpp:94-98)
  if (!rc) rc = kkamd_sptrsv_symbolic(q->hl, L->num_rows, L->d_row_map, (const int32_t*)L->d_entries, L->offset_type, stream);
  if (!rc) rc = kkamd_sptrsv_symbolic(q->hu, U->num_rows, U->d_row_map, (const int32_t*)U->d_entries, U->offset_type, stream);
  if (!rc && hipMalloc(&q->d_tmp, (size_t)(L->num_rows ? L->num_rows : 1) * 8) != hipSuccess)
    rc = fail(KKAMD_ERR_ALLOC, "kkamd_precond_create_lu: hipMalloc of %lld bytes failed", (long long)L->num_rows * 8);
  if (rc) { kkamd_precond_destroy(q); return rc; }
  *p = q;
  return KKAMD_OK;
}

extern "C" int kkamd_precond_create_callback(kkamd_precond_t** p, kkamd_precond_fn fn, void* ctx) {
  if (!p || !fn) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_precond_create_callback: null argument");
  kkamd_precond* q = new (std::nothrow) kkamd_precond;
  if (!q) return fail(KKAMD_ERR_ALLOC, "kkamd_precond_create_callback: out of host memory");
  q->kind = 2; q->fn = fn; q->ctx = ctx;
  *p = q;
  return KKAMD_OK;
}

extern "C" int kkamd_precond_destroy(kkamd_precond_t* p) {
  if (!p) return KKAMD_OK;
  if (p->plan) kkamd_spmv_plan_destroy(p->plan);
  if (p->hl) kkamd_sptrsv_destroy(p->hl);
  if (p->hu) kkamd_sptrsv_destroy(p->hu);
  if (p->d_tmp) (void)hipFree(p->d_tmp);
  delete p;
  return KKAMD_OK;
}

extern "C" int kkamd_precond_apply(kkamd_precond_t* p, const void* d_x, void* d_y, double alpha, double beta, int value_type,
                                   kkamd_stream_t stream) {
  if (!p) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_precond_apply: null preconditioner");
  if (value_type != KKAMD_F64 && value_type != KKAMD_F32) return fail(KKAMD_ERR_UNSUPPORTED, "kkamd_precond_apply: value type %d", value_type);
  if (p->kind == 2) return p->fn(p->ctx, d_x, d_y, alpha, beta, value_type, stream);
  if (p->kind == 0) {
    if (p->M.value_type != value_type) return fail(KKAMD_ERR_UNSUPPORTED, "kkamd_precond_apply: MatrixPrec type pair (%d, %d)", p->M.value_type, value_type);
    return kkamd_spmv(p->plan, &p->M, 'N', alpha, d_x, beta, d_y, value_type, stream);
  }
  if (p->L.value_type != value_type) return fail(KKAMD_ERR_UNSUPPORTED, "kkamd_precond_apply: LUPrec type pair (%d, %d)", p->L.value_type, value_type);
  const int64_t n = p->L.num_rows;
  if (int rc = kkamd_sptrsv_solve(p->hl, n, p->L.d_row_map, (const int32_t*)p->L.d_entries, p->L.d_values, d_x, p->d_tmp, p->L.offset_type,
                                  value_type, stream)) return rc;
  if (int rc = kkamd_sptrsv_solve(p->hu, n, p->U.d_row_map, (const int32_t*)p->U.d_entries, p->U.d_values, p->d_tmp, p->d_tmp, p->U.offset_type,
                                  value_type, stream)) return rc;
  // KokkosBlas::axpby(alpha, _tmp2, beta, Y) (LUPrec.hpp:100); beta == 0 does not read y
  const void* yy = beta == 0.0 ? nullptr : d_y;
  return value_type == KKAMD_F64 ? gm_axpby<double>(n, alpha, p->d_tmp, beta, yy, d_y, to_hip(stream))
                                 : gm_axpby<float>(n, alpha, p->d_tmp, beta, yy, d_y, to_hip(stream));
}

// ------------------------------------------------------------------------------------------------------------------------------------
// the handle
// ------------------------------------------------------------------------------------------------------------------------------------
struct kkamd_gmres_handle {
  int64_t m = 50, max_restart = 50;
  double tol = 1e-8;
  int ortho = 0, verbose = 0, fuse = 1, rows_per_group = 0, profile = 0, fuse_max_k = kGmFuseDefaultK;
  // results of the last solve
  int64_t num_iters = -1, cycles = 0, host_syncs = 0, launches = 0, last_fused = 0;
  double end_rel_res = -1;
  int conv_flag = KKAMD_GMRES_NOT_RUN;
  std::vector<double> short_res, true_res, H;   // H: (m_alloc + 1) x m_alloc, column-major, un-rotated, last cycle
  std::vector<double> t_precond, t_spmv, t_ortho; // knob "profile": milliseconds per iteration of the last solve, from events on the stream
  // workspace, kept while n, m and the value type stay
  int64_t n_alloc = -1, m_alloc = -1, groups_alloc = 0;
  int type_alloc = -1;
  void *V = nullptr, *work[4] = {nullptr, nullptr, nullptr, nullptr}, *P1 = nullptr, *P2 = nullptr, *SSw = nullptr, *SSr = nullptr, *d_h = nullptr;
  int64_t bytes = 0;
  // the SpMV plan of the matrix last solved with
  kkamd_spmv_plan_t* plan = nullptr;
  kkamd_crs_t planA{};

  void free_work() {
    void** all[] = {&V, &work[0], &work[1], &work[2], &work[3], &P1, &P2, &SSw, &SSr, &d_h};
    for (void** q : all) { if (*q) (void)hipFree(*q); *q = nullptr; }
    n_alloc = m_alloc = -1; type_alloc = -1; bytes = 0; groups_alloc = 0;
  }
  void free_plan() { if (plan) kkamd_spmv_plan_destroy(plan); plan = nullptr; }
};

static int gm_alloc(void** p, size_t bytes, int64_t* total) {
  if (hipMalloc(p, bytes ? bytes : 1) != hipSuccess) return fail(KKAMD_ERR_ALLOC, "kkamd_gmres: hipMalloc of %zu bytes failed", bytes);
  *total += (int64_t)bytes;
  return KKAMD_OK;
}

// workspace for n rows, up to kmax columns per slab, the given groups
static int gm_ensure(kkamd_gmres_handle* h, int64_t n, int64_t m, int type, int64_t groups) {
  if (h->n_alloc == n && h->m_alloc == m && h->type_alloc == type && h->groups_alloc >= groups) return KKAMD_OK;
  h->free_work();
  const size_t vb = type == KKAMD_F64 ? 8 : 4, nn = (size_t)(n ? n : 1);
  int rc = gm_alloc(&h->V, nn * (size_t)(m + 1) * vb, &h->bytes);
  for (int i = 0; i < 4 && !rc; ++i) rc = gm_alloc(&h->work[i], nn * vb, &h->bytes);
  if (!rc) rc = gm_alloc(&h->P1, (size_t)groups * (size_t)(m + 1) * vb, &h->bytes);
  if (!rc) rc = gm_alloc(&h->P2, (size_t)groups * (size_t)(m + 1) * vb, &h->bytes);
  if (!rc) rc = gm_alloc(&h->SSw, (size_t)groups * vb, &h->bytes);
  if (!rc) rc = gm_alloc(&h->SSr, (size_t)groups * vb, &h->bytes);
  if (!rc) rc = gm_alloc(&h->d_h, (size_t)(3 * (m + 2)) * vb, &h->bytes);   // h1 | h2 | h, nrm
  if (rc) { h->free_work(); return rc; }
  h->n_alloc = n; h->m_alloc = m; h->type_alloc = type; h->groups_alloc = groups;
  return KKAMD_OK;
}

extern "C" int kkamd_gmres_create(kkamd_gmres_handle_t** handle, int64_t m, double tol, int64_t max_restart) {
  if (!handle) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_create: null handle pointer");
  if (m <= 0) return fail(KKAMD_ERR_INVALID_ARG, "gmres: Please choose restart size m greater than zero.");
  kkamd_gmres_handle* h = new (std::nothrow) kkamd_gmres_handle;
  if (!h) return fail(KKAMD_ERR_ALLOC, "kkamd_gmres_create: out of host memory");
  h->m = m; h->tol = tol; h->max_restart = max_restart;
  *handle = h;
  return KKAMD_OK;
}

extern "C" int kkamd_gmres_destroy(kkamd_gmres_handle_t* h) {
  if (!h) return KKAMD_OK;
  h->free_work(); h->free_plan();
  delete h;
  return KKAMD_OK;
}

extern "C" int kkamd_gmres_set(kkamd_gmres_handle_t* h, const char* key, int64_t value) {
  if (!h || !key) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_set: null argument");
  const std::string k(key);
  if (k == "ortho") { if (value != 0 && value != 1) return fail(KKAMD_ERR_INVALID_ARG, "Invalid argument for 'ortho'.  Please use 'CGS2' or 'MGS'."); h->ortho = (int)value; }
  else if (k == "verbose") h->verbose = value != 0;
  else if (k == "m") { if (value <= 0) return fail(KKAMD_ERR_INVALID_ARG, "gmres: Please choose restart size m greater than zero."); h->m = value; }
  else if (k == "max_restart") { if (value < 0) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_set: max_restart %lld", (long long)value); h->max_restart = value; }
  else if (k == "fuse") { if (value != 0 && value != 1) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_set: fuse is 0 or 1"); h->fuse = (int)value; }
  else if (k == "rows_per_group") {
    if (value != 0 && (value < 64 || value > (1 << 24) || value % 64)) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_set: rows_per_group is 0 or a multiple of 64 up to 2^24");
    h->rows_per_group = (int)value;
  } else if (k == "fuse_max_k") {
    if (value < 1 || value > kGmFuseMaxK) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_set: fuse_max_k is 1..%d", kGmFuseMaxK);
    h->fuse_max_k = (int)value;
  } else if (k == "profile") h->profile = value != 0;
  else return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_set: unknown key '%s'", key);
  return KKAMD_OK;
}

extern "C" int kkamd_gmres_set_tol(kkamd_gmres_handle_t* h, double tol) {
  if (!h) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_set_tol: null handle");
  h->tol = tol;
  return KKAMD_OK;
}

extern "C" int kkamd_gmres_reset(kkamd_gmres_handle_t* h, int64_t m, double tol, int64_t max_restart) {
  if (!h) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_reset: null handle");
  if (m <= 0) return fail(KKAMD_ERR_INVALID_ARG, "gmres: Please choose restart size m greater than zero.");
  h->m = m; h->tol = tol; h->max_restart = max_restart; h->ortho = 0; h->verbose = 0;
  h->num_iters = -1; h->end_rel_res = -1; h->conv_flag = KKAMD_GMRES_NOT_RUN;
  return KKAMD_OK;
}

extern "C" int kkamd_gmres_get(const kkamd_gmres_handle_t* h, const char* key, int64_t* value) {
  if (!h || !key || !value) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_get: null argument");
  const std::string k(key);
  if (k == "num_iters") *value = h->num_iters;
  else if (k == "conv_flag") *value = h->conv_flag;
  else if (k == "cycles") *value = h->cycles;
  else if (k == "host_syncs") *value = h->host_syncs;
  else if (k == "launches") *value = h->launches;
  else if (k == "plan_bytes") {
    int64_t pb = 0;
    if (h->plan) (void)kkamd_spmv_plan_query(h->plan, "plan_bytes", &pb);
    *value = h->bytes + pb;
  }
  else if (k == "ortho") *value = h->ortho;
  else if (k == "verbose") *value = h->verbose;
  else if (k == "m") *value = h->m;
  else if (k == "max_restart") *value = h->max_restart;
  else if (k == "fuse") *value = h->fuse;
  else if (k == "rows_per_group") *value = h->rows_per_group;
  else if (k == "profile") *value = h->profile;
  else if (k == "last_fused") *value = h->last_fused;
  else if (k == "fuse_max_k") *value = h->fuse_max_k;
  else if (k == "num_short_residuals") *value = (int64_t)h->short_res.size();
  else if (k == "num_true_residuals") *value = (int64_t)h->true_res.size();
  else if (k == "num_rows") *value = h->n_alloc < 0 ? 0 : h->n_alloc;
  else return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_get: unknown key '%s'", key);
  return KKAMD_OK;
}

extern "C" int kkamd_gmres_get_real(const kkamd_gmres_handle_t* h, const char* key, double* value) {
  if (!h || !key || !value) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_get_real: null argument");
  const std::string k(key);
  if (k == "end_rel_res") *value = h->end_rel_res;
  else if (k == "tol") *value = h->tol;
  else return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_get_real: unknown key '%s'", key);
  return KKAMD_OK;
}

extern "C" int kkamd_gmres_export(const kkamd_gmres_handle_t* h, const char* what, double* h_out, int64_t count) {
  if (!h || !what || (!h_out && count > 0)) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_export: null argument");
  const std::string k(what);
  const std::vector<double>* src = k == "short_residuals" ? &h->short_res : k == "true_residuals" ? &h->true_res : k == "hessenberg" ? &h->H
                                   : k == "precond_ms" ? &h->t_precond : k == "spmv_ms" ? &h->t_spmv : k == "ortho_ms" ? &h->t_ortho : nullptr;
  if (src) {
    if (count != (int64_t)src->size()) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_export: '%s' has %zu entries, count is %lld", what, src->size(), (long long)count);
    if (count) std::memcpy(h_out, src->data(), (size_t)count * 8);
    return KKAMD_OK;
  }
  if (k != "basis") return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_export: unknown array '%s'", what);
  if (h->n_alloc < 0) return fail(KKAMD_ERR_STATE, "kkamd_gmres_export: no solve has run");
  const int64_t total = h->n_alloc * (h->m_alloc + 1);
  if (count != total) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_export: 'basis' has %lld entries, count is %lld", (long long)total, (long long)count);
  if (!total) return KKAMD_OK;
  if (h->type_alloc == KKAMD_F64) { KK_HIP(hipMemcpy(h_out, h->V, (size_t)total * 8, hipMemcpyDeviceToHost)); return KKAMD_OK; }
  std::vector<float> tmp((size_t)total);
  KK_HIP(hipMemcpy(tmp.data(), h->V, (size_t)total * 4, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < total; ++i) h_out[i] = (double)tmp[(size_t)i];
  return KKAMD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------------------------------------------
namespace {

template <class T> struct Gm {
  kkamd_gmres_handle* h;
  hipStream_t st;
  int64_t n, R, G;

  int dot(int k, const T* V, int64_t ldv, const T* w, T* P) {
    KK_LAUNCH(gm_dot_kernel<T>, G, kBlock, 0, st, n, k, V, ldv, w, R, P);
    KK_LAUNCH_CHECK(); ++h->launches;
    return KKAMD_OK;
  }
  int update(int k, T alpha, const T* V, int64_t ldv, const T* Pin, int64_t gin, T* h_out, const T* hadd, T* hsum, const T* w_in, T* w_out, T* SS) {
    KK_LAUNCH(gm_update_kernel<T>, G, kBlock, (size_t)(k ? k : 1) * sizeof(T), st, n, k, alpha, V, ldv, Pin, gin, h_out, hadd, hsum, w_in, w_out, R, SS);
    KK_LAUNCH_CHECK(); ++h->launches;
    return KKAMD_OK;
  }
  bool can_fuse(int k) const { return h->fuse && k >= 1 && k <= h->fuse_max_k; }
  int fused(int k, T alpha, const T* V, int64_t ldv, const T* Pin, int64_t gin, T* h_out, const T* w_in, T* w_out, T* P2) {
    const int TR = gm_tile_rows(k, sizeof(T));
    const size_t smem = ((size_t)5 * k + (size_t)k * TR) * sizeof(T);
    switch ((k + kGmBatch - 1) / kGmBatch) {
#define KK_GM_CASE(NB) case NB: KK_LAUNCH((gm_fused_kernel<T, NB>), G, kBlock, smem, st, n, k, alpha, V, ldv, Pin, gin, h_out, w_in, w_out, R, TR, P2); break;
      KK_GM_CASE(1) KK_GM_CASE(2) KK_GM_CASE(3) KK_GM_CASE(4) KK_GM_CASE(5) KK_GM_CASE(6) KK_GM_CASE(7) KK_GM_CASE(8)
#undef KK_GM_CASE
      default: return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres: fused kernel asked for %d columns", k);
    }
    KK_LAUNCH_CHECK(); ++h->launches; h->last_fused = 1;
    return KKAMD_OK;
  }
  int normalise(const T* SS, T* nrm_out, int guard, const T* w, T* out) {
    KK_LAUNCH(gm_normalise_kernel<T>, out ? G : 1, kBlock, 0, st, n, SS, G, nrm_out, guard, w, out, R);
    KK_LAUNCH_CHECK(); ++h->launches;
    return KKAMD_OK;
  }
  int axpby(T a, const T* x, T b, const T* y, T* out, T* SS) {
    KK_LAUNCH(gm_axpby_kernel<T>, G, kBlock, 0, st, n, a, x, b, y, out, R, SS);
    KK_LAUNCH_CHECK(); ++h->launches;
    return KKAMD_OK;
  }
  int reduce(const T* P, int k, T* out) {
    KK_LAUNCH(gm_reduce_kernel<T>, 1, kBlock, 0, st, P, G, k, out);
    KK_LAUNCH_CHECK(); ++h->launches;
    return KKAMD_OK;
  }
  int sync() { KK_HIP(hipStreamSynchronize(st)); ++h->host_syncs; return KKAMD_OK; }
};

#define KK_TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

template <class T>
int gm_solve(kkamd_gmres_handle* h, const kkamd_crs_t* A, const T* B, T* X, kkamd_precond_t* precond, int vt, kkamd_stream_t stream) {
  const int64_t n = A->num_rows;
  const int m = (int)h->m;
  const int64_t maxRestart = h->max_restart;
  const T tol = (T)h->tol;
  const bool verbose = h->verbose != 0;
  if (m + 1 > kGmMaxK) return fail(KKAMD_ERR_UNSUPPORTED, "kkamd_gmres_solve: m = %d is above %d", m, kGmMaxK - 1);
  Gm<T> k{h, to_hip(stream), n, gm_rows_per_group(n, h->rows_per_group), 0};
  k.G = gm_groups(n, k.R);
  KK_TRY(gm_ensure(h, n, m, vt, k.G));
  // the plan belongs to one matrix (kkamd.h, SpMV): a new one when the arrays or extents differ from the last solve's
  if (h->plan && std::memcmp(&h->planA, A, sizeof(kkamd_crs_t)) != 0) h->free_plan();
  if (!h->plan && A->nnz > 0) { KK_TRY(kkamd_spmv_plan_create(&h->plan, A, KKAMD_SPMV_DEFAULT, stream)); h->planA = *A; }
  h->host_syncs = h->launches = 0; h->cycles = 0; h->last_fused = 0;
  h->short_res.clear(); h->true_res.clear();
  h->t_precond.clear(); h->t_spmv.clear(); h->t_ortho.clear();
  h->H.assign((size_t)(m + 1) * m, 0.0);

  T* V = (T*)h->V; T* Xiter = (T*)h->work[0]; T* Res = (T*)h->work[1]; T* Wj = (T*)h->work[2]; T* Wj2 = (T*)h->work[3];
  T* P1 = (T*)h->P1; T* P2 = (T*)h->P2; T* SSw = (T*)h->SSw; T* SSr = (T*)h->SSr;
  T* d_h1 = (T*)h->d_h; T* d_h2 = d_h1 + (m + 2); T* d_hh = d_h2 + (m + 2);
  const int64_t ldv = n ? n : 1;
  const size_t vb = sizeof(T);
  hipStream_t st = k.st;
  auto spmv = [&](const T* x, T* y) { return kkamd_spmv(h->plan, A, 'N', 1.0, x, 0.0, y, vt, stream); };

#ifndef KK_EMU
  struct Events {                                      // knob "profile": four marks per iteration, read after the iteration's synchronisation
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  } ev;
  if (h->profile) {
    ev.on = true;
    for (hipEvent_t& x : ev.e) KK_HIP(hipEventCreate(&x));
  }
#define KK_GM_MARK(i) do { if (ev.on) KK_HIP(hipEventRecord(ev.e[i], st)); } while (0)
#else
#define KK_GM_MARK(i) do { } while (0)
#endif
  bool converged = false;
  int64_t cycle = 0, numIters = 0;
  T nrmB, trueRes, relRes, shortRelRes;
  if (verbose) {
    std::printf("Starting GMRES with...\n  n:          %lld\n  m:          %d\n  maxRestart: %lld\n  tol:        %g\n  ortho:      %s\n  precond:    %s\n",
                (long long)n, m, (long long)maxRestart, (double)tol, h->ortho == 0 ? "CGS2" : "MGS", precond ? "ON" : "OFF");
  }
  KK_HIP(hipMemsetAsync(Xiter, 0, (size_t)(n ? n : 1) * vb, st));   // Xiter("Xiter", n) is zero-initialised (:97)
  // nrmB and the initial true residual (:118-124), one synchronisation for both
  T hbuf[2];
  KK_TRY(k.axpby(T(1), B, T(0), nullptr, nullptr, SSr));
  KK_TRY(k.normalise(SSr, d_hh, 0, nullptr, nullptr));
  KK_TRY(spmv(X, Wj));
  KK_TRY(k.axpby(T(1), B, T(-1), Wj, Res, SSr));
  KK_TRY(k.normalise(SSr, d_hh + 1, 0, nullptr, nullptr));
  KK_HIP(hipMemcpyAsync(hbuf, d_hh, 2 * vb, hipMemcpyDeviceToHost, st));
  KK_TRY(k.sync());
  nrmB = hbuf[0]; trueRes = hbuf[1];
  if (nrmB != 0) relRes = trueRes / nrmB;
  else if (trueRes == 0) relRes = trueRes;
  else { KK_HIP(hipMemsetAsync(X, 0, (size_t)n * vb, st)); relRes = 0; }   // B is zero, but X has wrong initial guess (:129-131)
  shortRelRes = relRes;
  h->true_res.push_back((double)relRes);
  if (verbose) std::printf("Initial relative residual is: %g\n", (double)relRes);
  // a NaN here (in b, x0 or A) would fall through the loop condition below and be reported as NoConv by the reference; this library
  // reports it the way the reference reports a NaN inside the loop (:224-226)
  if (std::isnan(relRes)) return fail(KKAMD_ERR_NUMERIC, "gmres: Relative residual is nan. Terminating solver.");
  if (relRes < tol) converged = true;

  std::vector<T> Hh((size_t)(m + 1) * m), GVec((size_t)m + 1), Cos((size_t)m), Sin((size_t)m), Ls((size_t)m), hcol((size_t)m + 2);
  auto Hat = [&](int i, int j) -> T& { return Hh[(size_t)j * (m + 1) + i]; };

  while (!converged && cycle <= maxRestart && shortRelRes >= 1e-14) {
    GVec[0] = trueRes;
    std::fill(Hh.begin(), Hh.end(), T(0));
    std::fill(h->H.begin(), h->H.end(), 0.0);
    // V0 = Res / norm(Res) (:145-147): the norm comes from the slab the residual evaluation left, the same value the host holds
    KK_TRY(k.normalise(SSr, nullptr, 0, Res, V));
    const T* Vj = V;
    for (int j = 0; j < m; ++j) {
      KK_GM_MARK(0);
      if (precond) {
        KK_TRY(kkamd_precond_apply(precond, Vj, Wj2, 1.0, 0.0, vt, stream));   // wj2 = M * Vj
        KK_GM_MARK(1);
        KK_TRY(spmv(Wj2, Wj));
      } else {
        KK_GM_MARK(1);
        KK_TRY(spmv(Vj, Wj));
      }
      KK_GM_MARK(2);
      const int kc = j + 1;
      T tmpNrm;
      if (h->ortho == 1) {                                                     // MGS (:157-163)
        for (int i = 0; i <= j; ++i) {
          const T* Vi = V + (int64_t)i * ldv;
          KK_TRY(k.dot(1, Vi, ldv, Wj, P1));
          KK_TRY(k.update(1, T(-1), Vi, ldv, P1, k.G, d_hh + i, nullptr, nullptr, Wj, Wj, i == j ? SSw : nullptr));
          if (i < j) {
            KK_HIP(hipMemcpyAsync(&hcol[i], d_hh + i, vb, hipMemcpyDeviceToHost, st));
            KK_TRY(k.sync());
          }
        }
        KK_TRY(k.normalise(SSw, d_hh + kc, 1, Wj, V + (int64_t)kc * ldv));
        KK_GM_MARK(3);
        KK_HIP(hipMemcpyAsync(&hcol[j], d_hh + j, 2 * vb, hipMemcpyDeviceToHost, st));
        KK_TRY(k.sync());
      } else {                                                                 // CGS2 (:164-178)
        KK_TRY(k.dot(kc, V, ldv, Wj, P1));
        if (k.can_fuse(kc)) {
          KK_TRY(k.fused(kc, T(-1), V, ldv, P1, k.G, d_h1, Wj, Wj, P2));
        } else {
          KK_TRY(k.update(kc, T(-1), V, ldv, P1, k.G, d_h1, nullptr, nullptr, Wj, Wj, nullptr));
          KK_TRY(k.dot(kc, V, ldv, Wj, P2));
        }
        KK_TRY(k.update(kc, T(-1), V, ldv, P2, k.G, d_h2, d_h1, d_hh, Wj, Wj, SSw));
        KK_TRY(k.normalise(SSw, d_hh + kc, 1, Wj, V + (int64_t)kc * ldv));
        KK_GM_MARK(3);
        KK_HIP(hipMemcpyAsync(hcol.data(), d_hh, (size_t)(kc + 1) * vb, hipMemcpyDeviceToHost, st));
        KK_TRY(k.sync());
      }
#ifndef KK_EMU
      if (ev.on) {                                                             // the copy of h is behind mark 3: the kernels alone are timed
        float a = 0, b = 0, c = 0;
        KK_HIP(hipEventSynchronize(ev.e[3]));
        KK_HIP(hipEventElapsedTime(&a, ev.e[0], ev.e[1])); KK_HIP(hipEventElapsedTime(&b, ev.e[1], ev.e[2])); KK_HIP(hipEventElapsedTime(&c, ev.e[2], ev.e[3]));
        h->t_precond.push_back(a); h->t_spmv.push_back(b); h->t_ortho.push_back(c);
      }
#endif
      for (int i = 0; i <= j; ++i) Hat(i, j) = hcol[i];
      tmpNrm = hcol[kc];
      Hat(j + 1, j) = tmpNrm;
      for (int i = 0; i <= j + 1; ++i) h->H[(size_t)j * (m + 1) + i] = (double)Hat(i, j);
      if (tmpNrm > 1e-14) Vj = V + (int64_t)kc * ldv;

      // Givens rotations and the shortcut residual (:194-213)
      for (int i = 0; i < j; ++i) {
        const T tempVal = Cos[i] * Hat(i, j) + Sin[i] * Hat(i + 1, j);
        Hat(i + 1, j) = -Sin[i] * Hat(i, j) + Cos[i] * Hat(i + 1, j);
        Hat(i, j) = tempVal;
      }
      const T f = Hat(j, j), g = Hat(j + 1, j);
      const T f2 = f * f, g2 = g * g;
      T fg2 = f2 + g2;
      const T D1 = T(1) / std::sqrt(f2 * fg2);
      Cos[j] = f2 * D1;
      fg2 = fg2 * D1;
      Hat(j, j) = f * fg2;
      Sin[j] = f * D1 * g;
      Hat(j + 1, j) = 0;
      GVec[j + 1] = GVec[j] * (-Sin[j]);
      GVec[j] = GVec[j] * Cos[j];
      shortRelRes = std::fabs(GVec[j + 1]) / nrmB;
      h->short_res.push_back((double)shortRelRes);
      if (verbose) std::printf("Shortcut relative residual for iteration %lld is: %g\n", (long long)(j + cycle * m), (double)shortRelRes);
      if (tmpNrm <= 1e-14 && shortRelRes >= tol)
        return fail(KKAMD_ERR_NUMERIC, "GMRES has experienced lucky breakdown, but the residual has not converged.\n"
                                       "                                  Solver terminated without convergence.");
      if (std::isnan(shortRelRes)) return fail(KKAMD_ERR_NUMERIC, "gmres: Relative residual is nan. Terminating solver.");

      if (shortRelRes < tol || j == m - 1) {                                   // check the true residual (:229-281)
        for (int i = 0; i < m; ++i) Ls[i] = GVec[i];
        for (int i = j; i >= 0; --i) {                                         // SerialTrsm "L", "U", "N", "N" on H(0..j, 0..j)
          T s = Ls[i];
          for (int c = i + 1; c <= j; ++c) s -= Hat(i, c) * Ls[c];
          Ls[i] = s / Hat(i, i);
        }
        KK_HIP(hipMemcpyAsync(d_h1, Ls.data(), (size_t)kc * vb, hipMemcpyHostToDevice, st));
        if (precond) {
          KK_TRY(k.update(kc, T(1), V, ldv, d_h1, 1, nullptr, nullptr, nullptr, nullptr, Wj, nullptr));   // wj = V(1:j+1) * lsSoln
          KK_HIP(hipMemcpyAsync(Xiter, X, (size_t)n * vb, hipMemcpyDeviceToDevice, st));
          KK_TRY(kkamd_precond_apply(precond, Wj, Xiter, 1.0, 1.0, vt, stream));                          // Xiter = M * wj + X
        } else {
          KK_TRY(k.update(kc, T(1), V, ldv, d_h1, 1, nullptr, nullptr, nullptr, X, Xiter, nullptr));      // x_iter = x + V(1:j+1) * lsSoln
        }
        KK_TRY(spmv(Xiter, Wj));
        KK_TRY(k.axpby(T(1), B, T(-1), Wj, Res, SSr));
        KK_TRY(k.normalise(SSr, d_hh, 0, nullptr, nullptr));
        KK_HIP(hipMemcpyAsync(hbuf, d_hh, vb, hipMemcpyDeviceToHost, st));
        KK_TRY(k.sync());                                                      // also orders the next copy into d_h1 after this update
        trueRes = hbuf[0];
        relRes = trueRes / nrmB;
        h->true_res.push_back((double)relRes);
        if (verbose) std::printf("True relative residual for iteration %lld is : %g\n", (long long)(j + cycle * m), (double)relRes);
        numIters = j + 1;
        if (relRes < tol) {
          converged = true;
          KK_HIP(hipMemcpyAsync(X, Xiter, (size_t)n * vb, hipMemcpyDeviceToDevice, st));
          break;
        } else if (shortRelRes < 1e-30) {
          if (verbose)
            std::printf("Short residual has converged to machine zero, but true residual is not converged.\n"
                        "You may have given GMRES a singular matrix. Ending the GMRES iteration.\n");
          break;
        }
      }
    }
    ++cycle;
    KK_HIP(hipMemcpyAsync(X, Xiter, (size_t)n * vb, hipMemcpyDeviceToDevice, st));
  }

  if (verbose) std::printf("Ending relative residual is: %g\n", (double)relRes);
  int flag;
  if (converged) { if (verbose) std::printf("Solver converged! \n"); flag = KKAMD_GMRES_CONV; }
  else if (shortRelRes < tol) { if (verbose) std::printf("Shortcut residual converged, but solver experienced a loss of accuracy.\n"); flag = KKAMD_GMRES_LOA; }
  else { if (verbose) std::printf("Solver did not converge. :( \n"); flag = KKAMD_GMRES_NO_CONV; }
  const int64_t num_iters = cycle > 0 ? (cycle - 1) * m + numIters : 0;
  if (verbose) std::printf("The solver completed %lld iterations.\n", (long long)num_iters);
  KK_HIP(hipStreamSynchronize(st));                                            // the solve returns counts, and X is final
  h->num_iters = num_iters; h->end_rel_res = (double)relRes; h->conv_flag = flag; h->cycles = cycle;
  return KKAMD_OK;
#undef KK_GM_MARK
}

template <class T>
int gm_dot_entry(kkamd_gmres_handle* h, int64_t n, int k, const T* V, int64_t ldv, const T* w, T* d_h, kkamd_stream_t stream) {
  Gm<T> g{h, to_hip(stream), n, gm_rows_per_group(n, h->rows_per_group), 0};
  g.G = gm_groups(n, g.R);
  DevBuf P;
  if (P.alloc((size_t)g.G * k * sizeof(T)) != hipSuccess) return fail(KKAMD_ERR_ALLOC, "kkamd_gmres_dot: hipMalloc failed");
  T* slab = P.as<T>();
  KK_TRY(g.dot(k, V, ldv, w, slab));
  KK_TRY(g.reduce(slab, k, d_h));
  KK_HIP(hipStreamSynchronize(g.st));                                          // the slab is freed on return
  return KKAMD_OK;
}

template <class T>
int gm_update_entry(kkamd_gmres_handle* h, int64_t n, int k, T alpha, const T* V, int64_t ldv, const T* d_y, const T* w_in, T* w_out, T* d_h2,
                    T* d_sumsq, kkamd_stream_t stream) {
  Gm<T> g{h, to_hip(stream), n, gm_rows_per_group(n, h->rows_per_group), 0};
  g.G = gm_groups(n, g.R);
  DevBuf P, SS;
  if (P.alloc((size_t)g.G * k * sizeof(T)) != hipSuccess || SS.alloc((size_t)g.G * sizeof(T)) != hipSuccess)
    return fail(KKAMD_ERR_ALLOC, "kkamd_gmres_update: hipMalloc failed");
  h->last_fused = 0;
  if (d_h2 && g.can_fuse(k)) {
    KK_TRY(g.fused(k, alpha, V, ldv, d_y, 1, nullptr, w_in, w_out, P.as<T>()));
    if (d_sumsq) KK_TRY(g.axpby(T(1), w_out, T(0), nullptr, nullptr, SS.as<T>()));
  } else {
    KK_TRY(g.update(k, alpha, V, ldv, d_y, 1, nullptr, nullptr, nullptr, w_in, w_out, d_sumsq ? SS.as<T>() : nullptr));
    if (d_h2) KK_TRY(g.dot(k, V, ldv, w_out, P.as<T>()));
  }
  if (d_h2) KK_TRY(g.reduce(P.as<T>(), k, d_h2));
  if (d_sumsq) KK_TRY(g.reduce(SS.as<T>(), 1, d_sumsq));
  KK_HIP(hipStreamSynchronize(g.st));
  return KKAMD_OK;
}

int gm_check_block(const char* who, const kkamd_gmres_handle_t* h, int64_t n, int64_t k, int64_t ldv, int value_type) {
  if (!h) return fail(KKAMD_ERR_INVALID_ARG, "%s: null handle", who);
  if (value_type != KKAMD_F64 && value_type != KKAMD_F32) return fail(KKAMD_ERR_UNSUPPORTED, "%s: value type %d", who, value_type);
  if (n < 1 || k < 1 || k > kGmMaxK || ldv < n) return fail(KKAMD_ERR_INVALID_ARG, "%s: n = %lld, k = %lld (1..%d), ldv = %lld", who, (long long)n, (long long)k, kGmMaxK, (long long)ldv);
  return KKAMD_OK;
}

}  // namespace

extern "C" int kkamd_gmres_dot(kkamd_gmres_handle_t* h, int64_t n, int64_t k, const void* d_V, int64_t ldv, const void* d_w, void* d_h, int value_type,
                               kkamd_stream_t stream) {
  KK_TRY(gm_check_block("kkamd_gmres_dot", h, n, k, ldv, value_type));
  return value_type == KKAMD_F64 ? gm_dot_entry<double>(h, n, (int)k, (const double*)d_V, ldv, (const double*)d_w, (double*)d_h, stream)
                                 : gm_dot_entry<float>(h, n, (int)k, (const float*)d_V, ldv, (const float*)d_w, (float*)d_h, stream);
}

extern "C" int kkamd_gmres_update(kkamd_gmres_handle_t* h, int64_t n, int64_t k, double alpha, const void* d_V, int64_t ldv, const void* d_h,
                                  const void* d_w_in, void* d_w_out, void* d_h2, void* d_sumsq, int value_type, kkamd_stream_t stream) {
  KK_TRY(gm_check_block("kkamd_gmres_update", h, n, k, ldv, value_type));
  return value_type == KKAMD_F64
             ? gm_update_entry<double>(h, n, (int)k, alpha, (const double*)d_V, ldv, (const double*)d_h, (const double*)d_w_in, (double*)d_w_out,
                                       (double*)d_h2, (double*)d_sumsq, stream)
             : gm_update_entry<float>(h, n, (int)k, (float)alpha, (const float*)d_V, ldv, (const float*)d_h, (const float*)d_w_in, (float*)d_w_out,
                                      (float*)d_h2, (float*)d_sumsq, stream);
}

extern "C" int kkamd_gmres_solve(kkamd_gmres_handle_t* h, const kkamd_crs_t* A, const void* d_b, void* d_x, kkamd_precond_t* precond,
                                 int vector_type, kkamd_stream_t stream) {
  if (!h || !A) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gmres_solve: null argument");
  KK_TRY(check_crs(A));
  // x has numCols entries and b numRows (the host layers check their views' extents against these before they unwrap them): what is left
  // of gmres.hpp:110-116 at this boundary is X.extent(0) != B.extent(0)
  if (A->num_cols != A->num_rows)
    return fail(KKAMD_ERR_INVALID_ARG, "KokkosSparse::gmres: Dimensions do not match: , A: %lld x %lld, x: %lld, b: %lld", (long long)A->num_rows,
                (long long)A->num_cols, (long long)A->num_cols, (long long)A->num_rows);
  if (A->value_type != vector_type || (vector_type != KKAMD_F64 && vector_type != KKAMD_F32))
    return fail(KKAMD_ERR_UNSUPPORTED, "kkamd_gmres_solve: type pair (%d, %d) is not supported: (F64,F64) or (F32,F32)", A->value_type, vector_type);
  TraceRange range("GMRES::TotalTime:");
  return vector_type == KKAMD_F64 ? gm_solve<double>(h, A, (const double*)d_b, (double*)d_x, precond, vector_type, stream)
                                  : gm_solve<float>(h, A, (const float*)d_b, (float*)d_x, precond, vector_type, stream);
}
