// kk_gauss_seidel.hip -- point multicolor Gauss-Seidel: KokkosSparse::gauss_seidel_symbolic / gauss_seidel_numeric /
// {symmetric,forward_sweep,backward_sweep}_gauss_seidel_apply (sparse/src/KokkosSparse_gauss_seidel.hpp; the native implementation is
// sparse/impl/KokkosSparse_gauss_seidel_impl.hpp: initialize_symbolic :697-830, the row update :159-179, point_apply :1401-1466, the
// sweep order :1496-1560) for a CRS matrix whose leading num_rows x num_rows block has its diagonal stored.
//
// Symbolic phase, on the device.
//   1. one pass validates every row (columns in [0, num_cols), exactly one diagonal entry) and records the diagonal's position;
//   2. when the graph is not declared symmetric it is transposed (kkamd_transpose, values NULL): a row's neighbours are read from A and
//      from the transpose, nothing is merged;
//   3. the rows are coloured.  Jones-Plassmann with the priority pair (h(i), i), h = gs_hash below: in each round every uncoloured row
//      whose uncoloured neighbours all have lower priority takes the smallest colour no coloured neighbour holds.  A round reads the
//      colours of the round before and writes a second array, so a round sees no colour of its own: colours and the number of rounds
//      are functions of the graph and h alone.  The colouring equals the sequential greedy colouring in descending priority, because a
//      row that has become a local maximum has exactly its higher-priority neighbours coloured.  One launch and one host
//      synchronisation (the count of rows still uncoloured) per round.  A caller's colours are validated in one pass instead;
//   4. the rows are grouped by colour, ascending inside a colour, the rows longer than long_row_threshold at the end of their colour
//      (segment 2 c of the grouped list holds the other rows of colour c + 1, segment 2 c + 1 its long rows: counted, scattered with
//      integer atomics, every segment sorted ascending);
//   5. the grouped list is the permutation.  The permuted graph is built: row offsets, renumbered columns (ghost columns keep their
//      index) in their original order inside the row, and per permuted row the offset of its source row, so that numeric is one gather.
// The colour sets fill a kk::LevelSchedule (kk_levels.h): a colour is a level, build_plan chains runs of narrow colours.
//
// Apply.  X and Y are copied into row-major permuted work buffers; one launch per colour over that colour's contiguous block of
// permuted rows: a group of LPR lanes owns a row, strides over its entries (column and value loads contiguous across the groups of a
// wave), gathers from the permuted X, reduces with kk::group_sum (fixed order) and its first lane writes
// x_i + omega * (y_i - sum) * inv_diag_i, the diagonal term part of the sum as in the reference.  The long rows at the end of a colour
// get a launch of their own with one wave per row; the reference's atomic_add over chunks (:181-196) is not reproduced: no floating-point
// atomic anywhere, the same bits on every run.  num_vecs > 1: the columns go in batches of kGsBatch = 4 held in registers, one batch
// per blockIdx.y, so the matrix is read once per batch; every column sums in the order of the rank-1 kernel.
// No work-item ever waits on another workgroup: every dependency between workgroups is a kernel boundary on the stream.
#include "kk_levels.h"
#include <climits>
#include <new>

namespace kk {

constexpr unsigned long long kGsNoError = ~0ull;
enum { kGsErrRowMap = 0, kGsErrColumn = 1, kGsErrNoDiag = 2, kGsErrManyDiag = 3, kGsErrNone = 7 };
constexpr int kGsLanes = 8;   // lanes per row of the analysis kernels
constexpr int kGsBatch = 4;   // columns of a multivector held in registers per sweep: fp64 accumulators for 4 columns keep the kernel
                              // under 64 VGPRs, and 4 columns of a row-major X row are one 32-byte (fp64) or 16-byte (fp32) piece

// the priority hash: x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16, all in 32-bit unsigned arithmetic
__host__ __device__ __forceinline__ uint32_t gs_hash(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
// (h(j), j) > (h(i), i)
__device__ __forceinline__ bool gs_higher(int32_t j, int32_t i) {
  const uint32_t hj = gs_hash((uint32_t)j), hi = gs_hash((uint32_t)i);
  return hj > hi || (hj == hi && j > i);
}

// f(j) for the neighbours j < n, j != r of row r that this lane owns: A's row, then the transposed graph's (t_rm NULL: A alone)
template <class OffT, class F>
__device__ __forceinline__ void gs_neighbours(int64_t r, int lane, int64_t n, const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                              const OffT* __restrict__ t_rm, const int32_t* __restrict__ t_ent, F f) {
  const int64_t e = (int64_t)rm[r + 1];
  for (int64_t p = (int64_t)rm[r] + lane; p < e; p += kGsLanes) {
    const int32_t j = ent[p];
    if (j < n && j != r) f(j);
  }
  if (!t_rm) return;
  const int64_t te = (int64_t)t_rm[r + 1];
  for (int64_t p = (int64_t)t_rm[r] + lane; p < te; p += kGsLanes) {
    const int32_t j = t_ent[p];
    if (j < n && j != r) f(j);
  }
}

// ctr[0]: min over the offending rows of row * 8 + kind
template <class OffT>
__global__ __launch_bounds__(kBlock) void gs_validate_kernel(int64_t n, int64_t ncols, const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                             int32_t* __restrict__ diagpos, unsigned long long* __restrict__ ctr) {
  const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kGsLanes;
  const int lane  = threadIdx.x & (kGsLanes - 1);
  const bool valid = r < n;
  int kind = kGsErrNone, ndiag = 0, dpos = -1;
  if (valid) {
    const int64_t s = (int64_t)rm[r], e = (int64_t)rm[r + 1];
    int64_t len = e - s;
    if (s < 0 || len < 0 || len > (int64_t)INT32_MAX) { kind = kGsErrRowMap; len = 0; }
    for (int64_t j = s + lane; j < s + len; j += kGsLanes) {
      const int64_t c = ent[j];
      if (c < 0 || c >= ncols) { if (kGsErrColumn < kind) kind = kGsErrColumn; }
      else if (c == r) { ++ndiag; dpos = (int)(j - s); }
    }
  }
  for (int o = kGsLanes >> 1; o > 0; o >>= 1) {            // every lane of the wave takes part, rows past the end included
    const int k2 = __shfl_xor(kind, o, 64), n2 = __shfl_xor(ndiag, o, 64), d2 = __shfl_xor(dpos, o, 64);
    kind = k2 < kind ? k2 : kind; ndiag += n2; dpos = d2 > dpos ? d2 : dpos;
  }
  if (!valid || lane != 0) return;
  if (kind == kGsErrNone && ndiag == 0) kind = kGsErrNoDiag;
  if (kind == kGsErrNone && ndiag > 1) kind = kGsErrManyDiag;
  if (kind != kGsErrNone) { atomicMin(&ctr[0], (unsigned long long)r * 8ull + (unsigned long long)kind); return; }
  diagpos[r] = dpos;
}

// One round of the colouring.  cur: the colours before the round (0 = none), next: after it; ctr[1] counts the rows left uncoloured,
// ctr[2] is the largest colour.  The loops that shuffle run the same number of times in every lane of a wave.
template <class OffT>
__global__ __launch_bounds__(kBlock) void gs_color_round_kernel(int64_t n, const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                                const OffT* __restrict__ t_rm, const int32_t* __restrict__ t_ent,
                                                                const int32_t* __restrict__ cur, int32_t* __restrict__ next,
                                                                unsigned long long* __restrict__ ctr) {
  const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kGsLanes;
  const int lane  = threadIdx.x & (kGsLanes - 1);
  const bool valid = r < n;
  const int32_t c0 = valid ? cur[r] : 1;
  const bool todo  = valid && c0 == 0;
  int is_max = 1;
  if (todo)
    gs_neighbours<OffT>(r, lane, n, rm, ent, t_rm, t_ent, [&](int32_t j) { if (cur[j] == 0 && gs_higher(j, (int32_t)r)) is_max = 0; });
  for (int o = kGsLanes >> 1; o > 0; o >>= 1) is_max &= __shfl_xor(is_max, o, 64);
  const bool pick = todo && is_max;
  int32_t colour = 0;
  for (int32_t base = 0;; base += 64) {                      // windows of 64 colours: base + 1 .. base + 64
    unsigned long long mask = 0;
    if (pick && colour == 0)
      gs_neighbours<OffT>(r, lane, n, rm, ent, t_rm, t_ent, [&](int32_t j) {
        const int32_t cj = cur[j];
        if (cj > base && cj <= base + 64) mask |= 1ull << (cj - base - 1);
      });
    for (int o = kGsLanes >> 1; o > 0; o >>= 1) mask |= __shfl_xor(mask, o, 64);
    if (pick && colour == 0 && mask != ~0ull) colour = base + __ffsll(~mask);
    if (!__any(pick && colour == 0)) break;
  }
  if (!valid || lane != 0) return;
  if (!todo) { next[r] = c0; return; }
  next[r] = colour;
  if (colour == 0) atomicAdd(&ctr[1], 1ull);
  else atomicMax(&ctr[2], (unsigned long long)colour);
}

// a caller's colours: ctr[0] min over the offending rows of row * 2 + kind (0: colour outside [1, n], 1: shared with a neighbour), ctr[2] max
template <class OffT>
__global__ __launch_bounds__(kBlock) void gs_check_colors_kernel(int64_t n, const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                                 const OffT* __restrict__ t_rm, const int32_t* __restrict__ t_ent,
                                                                 const int32_t* __restrict__ colors, unsigned long long* __restrict__ ctr) {
  const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kGsLanes;
  const int lane  = threadIdx.x & (kGsLanes - 1);
  const bool valid = r < n;
  unsigned long long bad = kGsNoError;
  int32_t c = 0;
  if (valid) {
    c = colors[r];
    if (c < 1 || c > n) bad = (unsigned long long)r * 2ull;
    else
      gs_neighbours<OffT>(r, lane, n, rm, ent, t_rm, t_ent, [&](int32_t j) {
        if (colors[j] == c) { const unsigned long long b = (unsigned long long)(j < r ? j : r) * 2ull + 1ull; bad = b < bad ? b : bad; }
      });
  }
  for (int o = kGsLanes >> 1; o > 0; o >>= 1) { const unsigned long long b2 = __shfl_xor(bad, o, 64); bad = b2 < bad ? b2 : bad; }
  if (!valid || lane != 0) return;
  if (bad != kGsNoError) atomicMin(&ctr[0], bad);
  else atomicMax(&ctr[2], (unsigned long long)c);
}

template <class OffT>
__device__ __forceinline__ int64_t gs_segment(const OffT* __restrict__ rm, const int32_t* __restrict__ colors, int64_t r, int64_t threshold, int64_t* len) {
  *len = (int64_t)rm[r + 1] - (int64_t)rm[r];
  return 2 * (int64_t)(colors[r] - 1) + (threshold > 0 && *len > threshold ? 1 : 0);
}

// seg[2 k] rows and seg[2 k + 1] entries of segment k
template <class OffT>
__global__ __launch_bounds__(kBlock) void gs_count_kernel(int64_t n, const OffT* __restrict__ rm, const int32_t* __restrict__ colors, int64_t threshold,
                                                          unsigned long long* __restrict__ seg) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n) return;
  int64_t len;
  const int64_t k = gs_segment<OffT>(rm, colors, r, threshold, &len);
  atomicAdd(&seg[2 * k], 1ull);
  atomicAdd(&seg[2 * k + 1], (unsigned long long)len);
}

template <class OffT>
__global__ __launch_bounds__(kBlock) void gs_scatter_kernel(int64_t n, const OffT* __restrict__ rm, const int32_t* __restrict__ colors, int64_t threshold,
                                                            unsigned long long* __restrict__ cursor, int32_t* __restrict__ grouped) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= n) return;
  int64_t len;
  const int64_t k = gs_segment<OffT>(rm, colors, r, threshold, &len);
  grouped[atomicAdd(&cursor[k], 1ull)] = (int32_t)r;
}

// permuted row p is row grouped[p]: its length (scanned into the permuted row offsets afterwards), where its entries start in A, its diagonal
template <class OffT>
__global__ __launch_bounds__(kBlock) void gs_perm_kernel(int64_t n, const int32_t* __restrict__ grouped, const OffT* __restrict__ rm,
                                                         const int32_t* __restrict__ diagpos, int32_t* __restrict__ old_to_new,
                                                         int64_t* __restrict__ p_rm, int64_t* __restrict__ src, int32_t* __restrict__ p_diag) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p > n) return;
  if (p == n) { p_rm[n] = 0; return; }
  const int32_t r = grouped[p];
  old_to_new[r] = (int32_t)p;
  p_rm[p]   = (int64_t)rm[r + 1] - (int64_t)rm[r];
  src[p]    = (int64_t)rm[r];
  p_diag[p] = diagpos[r];
}

__global__ __launch_bounds__(kBlock) void gs_fill_kernel(int64_t n, const int64_t* __restrict__ p_rm, const int64_t* __restrict__ src,
                                                         const int32_t* __restrict__ ent, const int32_t* __restrict__ old_to_new,
                                                         int32_t* __restrict__ p_ent) {
  const int64_t p = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kGsLanes;
  const int lane  = threadIdx.x & (kGsLanes - 1);
  if (p >= n) return;
  const int64_t s = p_rm[p], len = p_rm[p + 1] - s, a = src[p];
  for (int64_t k = lane; k < len; k += kGsLanes) {
    const int32_t c = ent[a + k];
    p_ent[s + k] = c < n ? old_to_new[c] : c;
  }
}

// numeric: the values in the permuted order and 1 / a_ii (or the caller's inverse diagonal) per permuted row
template <class VT>
__global__ __launch_bounds__(kBlock) void gs_numeric_kernel(int64_t n, const int64_t* __restrict__ p_rm, const int64_t* __restrict__ src,
                                                            const int32_t* __restrict__ p_diag, const int32_t* __restrict__ grouped,
                                                            const VT* __restrict__ val, const VT* __restrict__ given_inv, VT* __restrict__ p_val,
                                                            VT* __restrict__ inv_diag) {
  const int64_t p = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kGsLanes;
  const int lane  = threadIdx.x & (kGsLanes - 1);
  if (p >= n) return;
  const int64_t s = p_rm[p], len = p_rm[p + 1] - s, a = src[p];
  for (int64_t k = lane; k < len; k += kGsLanes) p_val[s + k] = val[a + k];
  if (lane == 0) inv_diag[p] = given_inv ? given_inv[grouped[p]] : VT(1) / val[a + p_diag[p]];
}

// rows [0, n) of a strided multivector go to their permuted place, rows [n, rows) (ghost columns) keep theirs; w is row-major
template <class VT>
__global__ __launch_bounds__(kBlock) void gs_permute_in_kernel(int64_t rows, int64_t n, int64_t nv, const int32_t* __restrict__ old_to_new,
                                                               const VT* __restrict__ v, int64_t rs, int64_t cs, VT* __restrict__ w) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= rows * nv) return;
  const int64_t i = idx / nv, c = idx - i * nv;
  const int64_t p = i < n ? (int64_t)old_to_new[i] : i;
  w[p * nv + c] = v[i * rs + c * cs];
}

template <class VT>
__global__ __launch_bounds__(kBlock) void gs_permute_out_kernel(int64_t rows, int64_t n, int64_t nv, const int32_t* __restrict__ old_to_new,
                                                                const VT* __restrict__ w, VT* __restrict__ v, int64_t rs, int64_t cs) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= rows * nv) return;
  const int64_t i = idx / nv, c = idx - i * nv;
  const int64_t p = i < n ? (int64_t)old_to_new[i] : i;
  v[i * rs + c * cs] = w[p * nv + c];
}

// One permuted row per group of lpr lanes (a power of two, 1..64), columns [v0, v0 + nb) of the row-major X and Y.  X of the row's
// columns of other colours was written by an earlier launch, or by this workgroup before its last barrier; columns of the row's own
// colour are the row itself only (the diagonal).  X is neither const nor __restrict__, so it is read with ordinary vector loads.
template <class VT, int NB>
__device__ __forceinline__ void gs_row(bool valid, int64_t row, int lane, int lpr, const int64_t* __restrict__ p_rm, const int32_t* __restrict__ p_ent,
                                       const VT* __restrict__ p_val, const VT* __restrict__ inv_diag, const VT* __restrict__ Y, VT* X, int64_t nv,
                                       int64_t v0, int nb, VT omega) {
  VT acc[NB];
  KK_UNROLL
  for (int b = 0; b < NB; ++b) acc[b] = VT(0);
  if (valid) {
    const int64_t s = p_rm[row], e = p_rm[row + 1];
    for (int64_t j = s + lane; j < e; j += lpr) {            // rows longer than one pass loop
      const VT a = p_val[j];
      const VT* xp = X + (int64_t)p_ent[j] * nv + v0;
      KK_UNROLL
      for (int b = 0; b < NB; ++b)
        if (NB == 1 || b < nb) acc[b] += a * xp[b];
    }
  }
  KK_UNROLL
  for (int b = 0; b < NB; ++b) acc[b] = group_sum(acc[b], lpr);
  if (valid && lane == 0) {
    const VT d = inv_diag[row];
    KK_UNROLL
    for (int b = 0; b < NB; ++b)
      if (NB == 1 || b < nb) {
        const int64_t at = row * nv + v0 + b;
        const VT sum = Y[at] - acc[b];
        X[at] = X[at] + omega * sum * d;
      }
  }
}

// permuted rows [beg, beg + cnt): one colour, or its long-row tail with lpr = 64
template <class VT, int NB>
__global__ __launch_bounds__(kBlock) void gs_color_kernel(int64_t beg, int64_t cnt, int lpr, int lpr_shift, const int64_t* __restrict__ p_rm,
                                                          const int32_t* __restrict__ p_ent, const VT* __restrict__ p_val,
                                                          const VT* __restrict__ inv_diag, const VT* __restrict__ Y, VT* X, int64_t nv, VT omega) {
  const int64_t g  = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> lpr_shift;
  const int64_t v0 = (int64_t)blockIdx.y * NB;
  const int64_t left = nv - v0;
  gs_row<VT, NB>(g < cnt, beg + g, threadIdx.x & (lpr - 1), lpr, p_rm, p_ent, p_val, inv_diag, Y, X, nv, v0, (int)(left < NB ? left : NB), omega);
}

// colours first, first + step, ... (nlev of them; step -1 in a backward sweep) in one workgroup; the barrier's workgroup-scope ordering
// is all X needs between them
template <class VT, int NB>
__global__ __launch_bounds__(kBlock) void gs_chain_kernel(const int64_t* __restrict__ level_off, int first, int nlev, int step, int lpr, int lpr_shift,
                                                          const int64_t* __restrict__ p_rm, const int32_t* __restrict__ p_ent,
                                                          const VT* __restrict__ p_val, const VT* __restrict__ inv_diag, const VT* __restrict__ Y,
                                                          VT* X, int64_t nv, VT omega) {
  const int lane = threadIdx.x & (lpr - 1), grp = threadIdx.x >> lpr_shift, ngrp = kBlock >> lpr_shift;
  const int64_t v0 = (int64_t)blockIdx.y * NB;
  const int64_t left = nv - v0;
  const int nb = (int)(left < NB ? left : NB);
  for (int k = 0, l = first; k < nlev; ++k, l += step) {
    const int64_t beg = level_off[l], cnt = level_off[l + 1] - beg;
    for (int64_t base = 0; base < cnt; base += ngrp)         // uniform trip count: every lane reaches the reduction
      gs_row<VT, NB>(base + grp < cnt, beg + base + grp, lane, lpr, p_rm, p_ent, p_val, inv_diag, Y, X, nv, v0, nb, omega);
    __syncthreads();
  }
}

}  // namespace kk

struct kkamd_gs_handle {
  int algorithm = 0;
  int64_t nrows = 0, ncols = 0, nnz = 0;
  bool symbolic_complete = false, numeric_complete = false;
  int long_row_threshold = 0;
  int64_t num_colors = 0, coloring_rounds = 0, long_rows = 0, tail_launches = 0;
  kk::LevelSchedule sched;                                   // a colour is a level; d_grouped is the permutation (new -> old)
  std::vector<int64_t> long_begin, short_entries;           // per colour: where its long rows begin, the entries of the rows before
  int32_t *d_colors = nullptr, *d_old_to_new = nullptr, *d_p_ent = nullptr, *d_p_diag = nullptr;
  int64_t *d_p_rm = nullptr, *d_src = nullptr;
  int value_type = -1;                                       // of d_p_val / d_inv_diag, and of the work buffers
  void *d_p_val = nullptr, *d_inv_diag = nullptr, *d_X = nullptr, *d_Y = nullptr;
  int64_t buf_vecs = 0;
  int buf_type = -1;
  bool have_y = false;

  static void release(void* p) { if (p) (void)hipFree(p); }
  void clear_numeric() {
    numeric_complete = have_y = false;
    release(d_p_val); release(d_inv_diag); release(d_X); release(d_Y);
    d_p_val = d_inv_diag = d_X = d_Y = nullptr;
    value_type = buf_type = -1;
    buf_vecs = 0;
  }
  void clear_symbolic() {
    clear_numeric();
    symbolic_complete = false;
    sched.clear();
    long_begin.clear(); short_entries.clear();
    release(d_colors); release(d_old_to_new); release(d_p_ent); release(d_p_diag); release(d_p_rm); release(d_src);
    d_colors = d_old_to_new = d_p_ent = d_p_diag = nullptr;
    d_p_rm = d_src = nullptr;
    num_colors = coloring_rounds = long_rows = tail_launches = nnz = 0;
  }
};

namespace kk {

// The launches of one sweep.  Lanes per row: the knob, else 1 under GS_PERMUTED, else pow2_covering of a quarter of the launch's mean
// row length, about four entries per lane.  The triangular solve covers the whole mean row; here every row of a colour is ready at
// once, a launch is wide, and the reduction's shuffles and the idle lanes of a partly filled group cost more than a lane's short loop:
// on the 27-point lattice (26.5 entries per row) 8 lanes measured 25 % faster than the covering 32 and 6 % faster than 16, on the
// 7-point lattice 2 lanes 13 % faster than the covering 8.  A colour with a long-row tail launches the tail on its own
// (one wave per row), so its lanes come from the rows before the tail.
static void gs_build_plan(kkamd_gs_handle* h) {
  LevelSchedule& s = h->sched;
  auto lanes = [h](int64_t entries, int64_t rows) {
    if (h->sched.lanes_per_row) return h->sched.lanes_per_row;
    if (h->algorithm == KKAMD_GS_PERMUTED) return 1;
    return pow2_covering(rows > 0 ? ceil_div(entries, 4 * rows) : 1);
  };
  build_plan(&s, s.chain_rows > 0, lanes);
  h->tail_launches = 0;
  for (LevelLaunch& q : s.plan) {
    if (q.chain || h->long_begin[q.first] == s.level_off[q.first + 1]) continue;
    h->tail_launches += 1;
    q.lpr = lanes(h->short_entries[q.first], h->long_begin[q.first] - s.level_off[q.first]);
  }
}

template <class OffT>
static int gs_symbolic_typed(kkamd_gs_handle* h, int64_t n, int64_t ncols, const OffT* rm, const int32_t* ent, int offset_type, bool symmetric,
                             const int32_t* given_colors, hipStream_t st) {
  kkamd_stream_t kst = reinterpret_cast<kkamd_stream_t>(st);
  DevBuf diag_b, ctr_b, trm_b, tent_b, col_a, col_b, seg_b, cursor_b, segoff_b, grouped_b, off_b, o2n_b, prm_b, src_b, pdiag_b, pent_b;
  KK_HIP(diag_b.alloc(sizeof(int32_t) * (size_t)n));
  KK_HIP(ctr_b.alloc(sizeof(unsigned long long) * 3));
  unsigned long long* ctr = ctr_b.as<unsigned long long>();
  const unsigned row_grid = (unsigned)ceil_div(n * kGsLanes, kBlock), thread_grid = (unsigned)ceil_div(n + 1, kBlock);
  // 1. validate
  KK_HIP(hipMemsetAsync(ctr, 0xFF, 8, st));
  KK_HIP(hipMemsetAsync(ctr + 1, 0, 16, st));
  int32_t* diagpos = diag_b.as<int32_t>();                   // raw pointers for the launches: a DevBuf does not copy
  KK_LAUNCH((gs_validate_kernel<OffT>), row_grid, kBlock, 0, st, n, ncols, rm, ent, diagpos, ctr);
  KK_LAUNCH_CHECK();
  unsigned long long hc[3] = {0, 0, 0};
  OffT h_nnz = 0;
  KK_HIP(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, st));
  KK_HIP(hipMemcpyAsync(&h_nnz, rm + n, sizeof(OffT), hipMemcpyDeviceToHost, st));
  KK_HIP(hipStreamSynchronize(st));
  if (hc[0] != kGsNoError) {
    static const char* const what[] = {"its row_map offsets are not ascending (or it has more than 2^31 - 1 entries)",
                                       "a column is outside [0, num_cols)", "it has no diagonal entry", "it has more than one diagonal entry"};
    return fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_symbolic: row %lld: %s", (long long)(hc[0] >> 3), what[hc[0] & 7]);
  }
  const int64_t nnz = (int64_t)h_nnz;
  // 2. the transposed graph, when a row of A may not show all its neighbours
  const OffT* t_rm = nullptr;
  const int32_t* t_ent = nullptr;
  if (!symmetric) {
    KK_HIP(trm_b.alloc(sizeof(OffT) * (size_t)(ncols + 1)));
    KK_HIP(tent_b.alloc(sizeof(int32_t) * (size_t)nnz));
    const int rc = kkamd_transpose(n, ncols, nnz, rm, ent, nullptr, offset_type, KKAMD_F64, trm_b.p, tent_b.as<int32_t>(), nullptr, kst);
    if (rc) return rc;
    t_rm = trm_b.as<OffT>(); t_ent = tent_b.as<int32_t>();
  }
  // 3. colours
  KK_HIP(col_a.alloc(sizeof(int32_t) * (size_t)n));
  int64_t rounds = 0, num_colors = 0;
  if (given_colors) {
    KK_HIP(hipMemcpyAsync(col_a.p, given_colors, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    const int32_t* given = col_a.as<int32_t>();
    KK_LAUNCH((gs_check_colors_kernel<OffT>), row_grid, kBlock, 0, st, n, rm, ent, t_rm, t_ent, given, ctr);
    KK_LAUNCH_CHECK();
    KK_HIP(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, st));
    KK_HIP(hipStreamSynchronize(st));
    if (hc[0] != kGsNoError)
      return fail(KKAMD_ERR_INVALID_ARG, (hc[0] & 1) ? "kkamd_gs_symbolic: row %lld: the given colours give it and an adjacent row one colour"
                                                     : "kkamd_gs_symbolic: row %lld: its given colour is outside [1, num_rows]", (long long)(hc[0] >> 1));
    num_colors = (int64_t)hc[2];
  } else {
    KK_HIP(col_b.alloc(sizeof(int32_t) * (size_t)n));
    KK_HIP(hipMemsetAsync(col_a.p, 0, sizeof(int32_t) * (size_t)n, st));
    int64_t left = n;
    while (left > 0) {                                       // at most n rounds: the uncoloured row of highest priority always takes a colour
      KK_HIP(hipMemsetAsync(ctr + 1, 0, 8, st));
      const int32_t* cur = col_a.as<int32_t>();
      int32_t* next = col_b.as<int32_t>();
      KK_LAUNCH((gs_color_round_kernel<OffT>), row_grid, kBlock, 0, st, n, rm, ent, t_rm, t_ent, cur, next, ctr);
      KK_LAUNCH_CHECK();
      KK_HIP(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, st));
      KK_HIP(hipStreamSynchronize(st));
      std::swap(col_a.p, col_b.p);
      ++rounds;
      if ((int64_t)hc[1] >= left) return fail(KKAMD_ERR_STATE, "kkamd_gs_symbolic: round %lld coloured no row (internal error)", (long long)rounds);
      left = (int64_t)hc[1];
    }
    col_b.reset();
    num_colors = (int64_t)hc[2];
  }
  trm_b.reset(); tent_b.reset();
  const int32_t* colors = col_a.as<int32_t>();
  // 4. group by colour, long rows last
  const int64_t C = num_colors, S = 2 * C, threshold = h->long_row_threshold;
  KK_HIP(seg_b.alloc(sizeof(unsigned long long) * (size_t)(2 * S)));
  KK_HIP(hipMemsetAsync(seg_b.p, 0, sizeof(unsigned long long) * (size_t)(2 * S), st));
  unsigned long long* d_seg = seg_b.as<unsigned long long>();
  KK_LAUNCH((gs_count_kernel<OffT>), thread_grid, kBlock, 0, st, n, rm, colors, threshold, d_seg);
  KK_LAUNCH_CHECK();
  std::vector<unsigned long long> seg((size_t)(2 * S));
  KK_HIP(hipMemcpyAsync(seg.data(), seg_b.p, sizeof(unsigned long long) * (size_t)(2 * S), hipMemcpyDeviceToHost, st));
  KK_HIP(hipStreamSynchronize(st));
  std::vector<int64_t> seg_off((size_t)(S + 1), 0), level_off((size_t)(C + 1), 0), level_entries((size_t)C, 0), long_begin((size_t)C, 0),
      short_entries((size_t)C, 0);
  int64_t total = 0, long_rows = 0, max_rows = 0;
  for (int64_t k = 0; k < S; ++k) seg_off[k + 1] = seg_off[k] + (int64_t)seg[2 * k];
  for (int64_t c = 0; c < C; ++c) {
    level_off[c + 1]  = seg_off[2 * c + 2];
    long_begin[c]     = seg_off[2 * c + 1];
    short_entries[c]  = (int64_t)seg[4 * c + 1];
    level_entries[c]  = (int64_t)(seg[4 * c + 1] + seg[4 * c + 3]);
    total            += level_entries[c];
    long_rows        += (int64_t)seg[4 * c + 2];
    if (level_off[c + 1] - level_off[c] > max_rows) max_rows = level_off[c + 1] - level_off[c];
  }
  if (seg_off[S] != n) return fail(KKAMD_ERR_STATE, "kkamd_gs_symbolic: the colours hold %lld rows, not %lld (internal error)", (long long)seg_off[S], (long long)n);
  KK_HIP(segoff_b.alloc(sizeof(int64_t) * (size_t)(S + 1)));
  KK_HIP(cursor_b.alloc(sizeof(int64_t) * (size_t)(S + 1)));
  KK_HIP(off_b.alloc(sizeof(int64_t) * (size_t)(C + 1)));
  KK_HIP(grouped_b.alloc(sizeof(int32_t) * (size_t)n));
  KK_HIP(hipMemcpyAsync(segoff_b.p, seg_off.data(), sizeof(int64_t) * (size_t)(S + 1), hipMemcpyHostToDevice, st));
  KK_HIP(hipMemcpyAsync(cursor_b.p, seg_off.data(), sizeof(int64_t) * (size_t)(S + 1), hipMemcpyHostToDevice, st));
  KK_HIP(hipMemcpyAsync(off_b.p, level_off.data(), sizeof(int64_t) * (size_t)(C + 1), hipMemcpyHostToDevice, st));
  unsigned long long* cursor = cursor_b.as<unsigned long long>();
  int32_t* grouped = grouped_b.as<int32_t>();
  KK_LAUNCH((gs_scatter_kernel<OffT>), thread_grid, kBlock, 0, st, n, rm, colors, threshold, cursor, grouped);
  KK_LAUNCH_CHECK();
  int rc = kkamd_sort_crs(S, segoff_b.p, grouped, nullptr, KKAMD_I64, KKAMD_F64, kst);   // ascending inside every segment
  if (rc) return rc;
  // 5. the permutation and the permuted graph
  KK_HIP(o2n_b.alloc(sizeof(int32_t) * (size_t)n));
  KK_HIP(prm_b.alloc(sizeof(int64_t) * (size_t)(n + 1)));
  KK_HIP(src_b.alloc(sizeof(int64_t) * (size_t)n));
  KK_HIP(pdiag_b.alloc(sizeof(int32_t) * (size_t)n));
  KK_HIP(pent_b.alloc(sizeof(int32_t) * (size_t)total));
  int32_t *o2n = o2n_b.as<int32_t>(), *p_diag = pdiag_b.as<int32_t>(), *p_ent = pent_b.as<int32_t>();
  int64_t *p_rm = prm_b.as<int64_t>(), *src = src_b.as<int64_t>();
  KK_LAUNCH((gs_perm_kernel<OffT>), thread_grid, kBlock, 0, st, n, (const int32_t*)grouped, rm, (const int32_t*)diagpos, o2n, p_rm, src, p_diag);
  KK_LAUNCH_CHECK();
  rc = kkamd_exclusive_scan(prm_b.p, n + 1, KKAMD_I64, kst);
  if (rc) return rc;
  KK_LAUNCH(gs_fill_kernel, row_grid, kBlock, 0, st, n, (const int64_t*)p_rm, (const int64_t*)src, ent, (const int32_t*)o2n, p_ent);
  KK_LAUNCH_CHECK();
  KK_HIP(hipStreamSynchronize(st));                          // the host vectors above were the sources of asynchronous copies
  h->sched.d_grouped   = (int32_t*)grouped_b.release();
  h->sched.d_level_off = (int64_t*)off_b.release();
  h->sched.level_off.swap(level_off);
  h->sched.level_entries.swap(level_entries);
  h->sched.max_level_rows = max_rows;
  h->long_begin.swap(long_begin);
  h->short_entries.swap(short_entries);
  h->d_colors     = (int32_t*)col_a.release();
  h->d_old_to_new = (int32_t*)o2n_b.release();
  h->d_p_ent      = (int32_t*)pent_b.release();
  h->d_p_diag     = (int32_t*)pdiag_b.release();
  h->d_p_rm       = (int64_t*)prm_b.release();
  h->d_src        = (int64_t*)src_b.release();
  h->num_colors = C; h->coloring_rounds = rounds; h->long_rows = long_rows; h->nnz = total;
  return KKAMD_OK;
}

template <class VT>
static int gs_numeric_typed(kkamd_gs_handle* h, const VT* val, const VT* given_inv, hipStream_t st) {
  const int64_t n = h->nrows;
  if (h->value_type != scalar_tag<VT>::value) {
    h->clear_numeric();
    KK_HIP(hipMalloc(&h->d_p_val, sizeof(VT) * (size_t)(h->nnz ? h->nnz : 1)));
    KK_HIP(hipMalloc(&h->d_inv_diag, sizeof(VT) * (size_t)(n ? n : 1)));
    h->value_type = scalar_tag<VT>::value;
  }
  if (n > 0) {
    KK_LAUNCH((gs_numeric_kernel<VT>), (unsigned)ceil_div(n * kGsLanes, kBlock), kBlock, 0, st, n, (const int64_t*)h->d_p_rm, (const int64_t*)h->d_src,
              (const int32_t*)h->d_p_diag, (const int32_t*)h->sched.d_grouped, val, given_inv, (VT*)h->d_p_val, (VT*)h->d_inv_diag);
    KK_LAUNCH_CHECK();
  }
  h->numeric_complete = true;
  return KKAMD_OK;
}

template <class VT, int NB>
static int gs_sweep(const kkamd_gs_handle* h, int64_t nv, VT omega, bool backward, hipStream_t st) {
  const LevelSchedule& s = h->sched;
  const unsigned nbatch = (unsigned)ceil_div(nv, NB);
  const int64_t* p_rm = h->d_p_rm;
  const int32_t* p_ent = h->d_p_ent;
  const VT *p_val = (const VT*)h->d_p_val, *inv = (const VT*)h->d_inv_diag, *Y = (const VT*)h->d_Y;
  VT* X = (VT*)h->d_X;
  const int64_t np = (int64_t)s.plan.size();
  for (int64_t k = 0; k < np; ++k) {
    const LevelLaunch& q = s.plan[backward ? np - 1 - k : k];
    const int sh = log2i(q.lpr);
    if (q.chain) {
      KK_LAUNCH((gs_chain_kernel<VT, NB>), dim3(1u, nbatch), kBlock, 0, st, (const int64_t*)s.d_level_off, backward ? q.first + q.nlev - 1 : q.first, q.nlev,
                backward ? -1 : 1, q.lpr, sh, p_rm, p_ent, p_val, inv, Y, X, nv, omega);
      continue;
    }
    const int64_t beg = s.level_off[q.first], mid = h->long_begin[q.first], end = s.level_off[q.first + 1];
    if (mid > beg)
      KK_LAUNCH((gs_color_kernel<VT, NB>), dim3((unsigned)ceil_div((mid - beg) * q.lpr, kBlock), nbatch), kBlock, 0, st, beg, mid - beg, q.lpr, sh, p_rm, p_ent,
                p_val, inv, Y, X, nv, omega);
    if (end > mid)                                           // the long rows: one wave each
      KK_LAUNCH((gs_color_kernel<VT, NB>), dim3((unsigned)ceil_div((end - mid) * kWave, kBlock), nbatch), kBlock, 0, st, mid, end - mid, kWave, 6, p_rm, p_ent,
                p_val, inv, Y, X, nv, omega);
  }
  KK_LAUNCH_CHECK();
  return KKAMD_OK;
}

template <class VT>
static int gs_apply_typed(kkamd_gs_handle* h, VT* x, int64_t xrs, int64_t xcs, const VT* y, int64_t yrs, int64_t ycs, int64_t nv, bool init_zero_x,
                          bool update_y, double omega, int num_iter, int direction, hipStream_t st) {
  const int64_t n = h->nrows, nc = h->ncols;
  if (h->buf_type != scalar_tag<VT>::value || h->buf_vecs != nv) {
    h->release(h->d_X); h->release(h->d_Y);
    h->d_X = h->d_Y = nullptr;
    h->have_y = false;
    h->buf_type = -1;
    KK_HIP(hipMalloc(&h->d_X, sizeof(VT) * (size_t)(nc > 0 ? nc * nv : 1)));
    KK_HIP(hipMalloc(&h->d_Y, sizeof(VT) * (size_t)(n > 0 ? n * nv : 1)));
    h->buf_type = scalar_tag<VT>::value;
    h->buf_vecs = nv;
  }
  const int32_t* o2n = h->d_old_to_new;
  if (update_y) {
    if (n > 0) KK_LAUNCH((gs_permute_in_kernel<VT>), (unsigned)ceil_div(n * nv, kBlock), kBlock, 0, st, n, n, nv, o2n, y, yrs, ycs, (VT*)h->d_Y);
    h->have_y = true;
  }
  if (nc > 0) {
    if (init_zero_x) KK_HIP(hipMemsetAsync(h->d_X, 0, sizeof(VT) * (size_t)(nc * nv), st));
    else KK_LAUNCH((gs_permute_in_kernel<VT>), (unsigned)ceil_div(nc * nv, kBlock), kBlock, 0, st, nc, n, nv, o2n, (const VT*)x, xrs, xcs, (VT*)h->d_X);
  }
  for (int it = 0; it < num_iter; ++it) {
    if (direction != KKAMD_GS_BACKWARD) {
      const int rc = nv == 1 ? gs_sweep<VT, 1>(h, nv, (VT)omega, false, st) : gs_sweep<VT, kGsBatch>(h, nv, (VT)omega, false, st);
      if (rc) return rc;
    }
    if (direction != KKAMD_GS_FORWARD) {
      const int rc = nv == 1 ? gs_sweep<VT, 1>(h, nv, (VT)omega, true, st) : gs_sweep<VT, kGsBatch>(h, nv, (VT)omega, true, st);
      if (rc) return rc;
    }
  }
  if (nc > 0) KK_LAUNCH((gs_permute_out_kernel<VT>), (unsigned)ceil_div(nc * nv, kBlock), kBlock, 0, st, nc, n, nv, o2n, (const VT*)h->d_X, x, xrs, xcs);
  KK_LAUNCH_CHECK();
  return KKAMD_OK;
}

static int gs_check_matrix(const kkamd_gs_handle* h, const char* who, int64_t num_rows, int64_t num_cols, int offset_type) {
  if (num_rows != h->nrows || num_cols != h->ncols)
    return fail(KKAMD_ERR_INVALID_ARG, "%s: %lld x %lld differs from the %lld x %lld of the symbolic phase", who, (long long)num_rows, (long long)num_cols,
                (long long)h->nrows, (long long)h->ncols);
  if (offset_type != KKAMD_I32 && offset_type != KKAMD_I64) return fail(KKAMD_ERR_INVALID_ARG, "%s: unknown offset_type %d", who, offset_type);
  return KKAMD_OK;
}

}  // namespace kk

extern "C" {

int kkamd_gs_create(kkamd_gs_handle_t** handle, int algorithm) {
  if (!handle) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_create: null handle pointer");
  *handle = nullptr;
  if (algorithm == KKAMD_GS_CLUSTER || algorithm == KKAMD_GS_TWOSTAGE)
    return kk::fail(KKAMD_ERR_UNSUPPORTED, "kkamd_gs_create: %s is not implemented (GS_DEFAULT, GS_PERMUTED and GS_TEAM are)",
                    algorithm == KKAMD_GS_CLUSTER ? "GS_CLUSTER" : "GS_TWOSTAGE");
  if (algorithm < KKAMD_GS_DEFAULT || algorithm > KKAMD_GS_TWOSTAGE) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_create: unknown GSAlgorithm %d", algorithm);
  kkamd_gs_handle* h = new (std::nothrow) kkamd_gs_handle();
  if (!h) return kk::fail(KKAMD_ERR_ALLOC, "kkamd_gs_create: out of host memory");
  h->algorithm = algorithm;
  *handle      = h;
  return KKAMD_OK;
}

int kkamd_gs_destroy(kkamd_gs_handle_t* h) {
  if (!h) return KKAMD_OK;
  h->clear_symbolic();
  delete h;
  return KKAMD_OK;
}

int kkamd_gs_symbolic(kkamd_gs_handle_t* h, int64_t num_rows, int64_t num_cols, const void* d_row_map, const int32_t* d_entries, int offset_type,
                      int is_graph_symmetric, const int32_t* d_colors, kkamd_stream_t stream) {
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_symbolic: null handle");
  if (num_rows < 0 || num_cols > (int64_t)INT32_MAX)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_symbolic: %lld x %lld is outside [0, 2^31)", (long long)num_rows, (long long)num_cols);
  if (num_cols < num_rows)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_symbolic: num_cols %lld is below num_rows %lld", (long long)num_cols, (long long)num_rows);
  if (offset_type != KKAMD_I32 && offset_type != KKAMD_I64) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_symbolic: unknown offset_type %d", offset_type);
  if (num_rows > 0 && (!d_row_map || !d_entries)) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_symbolic: null pointer");
  kk::TraceRange range("KokkosSparse::gauss_seidel_symbolic[TPL_KKAMD]");
  hipStream_t st = kk::to_hip(stream);
  h->clear_symbolic();                                       // a repeated call analyses again
  h->nrows = num_rows;
  h->ncols = num_cols;
  if (num_rows == 0) {
    KK_HIP(hipStreamSynchronize(st));
    h->sched.level_off.assign(1, 0);
  } else {
    const int rc = offset_type == KKAMD_I64
                       ? kk::gs_symbolic_typed<int64_t>(h, num_rows, num_cols, (const int64_t*)d_row_map, d_entries, offset_type, is_graph_symmetric != 0, d_colors, st)
                       : kk::gs_symbolic_typed<int32_t>(h, num_rows, num_cols, (const int32_t*)d_row_map, d_entries, offset_type, is_graph_symmetric != 0, d_colors, st);
    if (rc) return rc;
  }
  kk::gs_build_plan(h);
  h->symbolic_complete = true;
  return KKAMD_OK;
}

int kkamd_gs_numeric(kkamd_gs_handle_t* h, int64_t num_rows, int64_t num_cols, const void* d_row_map, const int32_t* d_entries, const void* d_values,
                     const void* d_inverse_diagonal, int offset_type, int value_type, kkamd_stream_t stream) {
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_numeric: null handle");
  if (!h->symbolic_complete) return kk::fail(KKAMD_ERR_STATE, "KokkosSparse::gauss_seidel_numeric: the symbolic phase has not been completed on this handle");
  if (value_type != KKAMD_F64 && value_type != KKAMD_F32)
    return kk::fail(KKAMD_ERR_UNSUPPORTED, "kkamd_gs_numeric: unsupported value_type %d: F64 and F32 are", value_type);
  const int rc = kk::gs_check_matrix(h, "kkamd_gs_numeric", num_rows, num_cols, offset_type);
  if (rc) return rc;
  if (num_rows > 0 && !d_values) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_numeric: null values");
  kk::TraceRange range(value_type == KKAMD_F64 ? "KokkosSparse::gauss_seidel_numeric[TPL_KKAMD,double]" : "KokkosSparse::gauss_seidel_numeric[TPL_KKAMD,float]");
  hipStream_t st = kk::to_hip(stream);
  if (value_type == KKAMD_F64) return kk::gs_numeric_typed<double>(h, (const double*)d_values, (const double*)d_inverse_diagonal, st);
  return kk::gs_numeric_typed<float>(h, (const float*)d_values, (const float*)d_inverse_diagonal, st);
}

int kkamd_gs_apply(kkamd_gs_handle_t* h, int64_t num_rows, int64_t num_cols, const void* d_row_map, const int32_t* d_entries, const void* d_values,
                   void* d_x, int64_t x_row_stride, int64_t x_col_stride, const void* d_y, int64_t y_row_stride, int64_t y_col_stride, int64_t num_vecs,
                   int init_zero_x, int update_y, double omega, int num_iter, int direction, int offset_type, int value_type, kkamd_stream_t stream) {
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_apply: null handle");
  if (!h->symbolic_complete) return kk::fail(KKAMD_ERR_STATE, "KokkosSparse::gauss_seidel_apply: the symbolic phase has not been completed on this handle");
  if (value_type != KKAMD_F64 && value_type != KKAMD_F32)
    return kk::fail(KKAMD_ERR_UNSUPPORTED, "kkamd_gs_apply: unsupported value_type %d: F64 and F32 are", value_type);
  int rc = kk::gs_check_matrix(h, "kkamd_gs_apply", num_rows, num_cols, offset_type);
  if (rc) return rc;
  if (direction < KKAMD_GS_FORWARD || direction > KKAMD_GS_SYMMETRIC) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_apply: unknown GSDirection %d", direction);
  if (num_vecs < 1 || num_iter < 0) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_apply: num_vecs %lld is below 1 or num_iter %d is negative", (long long)num_vecs, num_iter);
  if ((num_cols > 0 && !d_x) || (num_rows > 0 && update_y && !d_y)) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_apply: null vector");
  if (h->numeric_complete && h->value_type != value_type)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_apply: value_type %d differs from the numeric phase's %d", value_type, h->value_type);
  if (!update_y && (!h->have_y || h->buf_vecs != num_vecs || h->buf_type != value_type))
    return kk::fail(KKAMD_ERR_STATE, "kkamd_gs_apply: update_y is false, but no earlier apply on this handle has stored a y with %lld vectors", (long long)num_vecs);
  hipStream_t st = kk::to_hip(stream);
  if (!h->numeric_complete) {                                // gauss_seidel_impl.hpp:1473
    rc = kkamd_gs_numeric(h, num_rows, num_cols, d_row_map, d_entries, d_values, nullptr, offset_type, value_type, stream);
    if (rc) return rc;
  }
  kk::TraceRange range(value_type == KKAMD_F64 ? "KokkosSparse::gauss_seidel_apply[TPL_KKAMD,double]" : "KokkosSparse::gauss_seidel_apply[TPL_KKAMD,float]");
  if (value_type == KKAMD_F64)
    return kk::gs_apply_typed<double>(h, (double*)d_x, x_row_stride, x_col_stride, (const double*)d_y, y_row_stride, y_col_stride, num_vecs, init_zero_x != 0,
                                      update_y != 0, omega, num_iter, direction, st);
  return kk::gs_apply_typed<float>(h, (float*)d_x, x_row_stride, x_col_stride, (const float*)d_y, y_row_stride, y_col_stride, num_vecs, init_zero_x != 0,
                                   update_y != 0, omega, num_iter, direction, st);
}

int kkamd_gs_set(kkamd_gs_handle_t* h, const char* key, int value) {
  if (!h || !key) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_set: null argument");
  if (std::string(key) == "long_row_threshold") {
    if (value < 0) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_set: long_row_threshold %d is negative", value);
    h->long_row_threshold = value;                           // read by the next symbolic call
    return KKAMD_OK;
  }
  const int rc = kk::set_knob(&h->sched, "kkamd_gs_set", key, value);
  if (rc) return rc;
  if (h->symbolic_complete) kk::gs_build_plan(h);
  return KKAMD_OK;
}

int kkamd_gs_get(const kkamd_gs_handle_t* h, const char* key, int64_t* value) {
  if (!h || !key || !value) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_get: null argument");
  const std::string k(key);
  if (kk::get_common(h->sched, k, value)) return KKAMD_OK;
  if (k == "num_colors") *value = h->num_colors;
  else if (k == "coloring_rounds") *value = h->coloring_rounds;
  else if (k == "num_rows") *value = h->nrows;
  else if (k == "num_cols") *value = h->ncols;
  else if (k == "symbolic_complete") *value = h->symbolic_complete ? 1 : 0;
  else if (k == "numeric_complete") *value = h->numeric_complete ? 1 : 0;
  else if (k == "algorithm") *value = h->algorithm;
  else if (k == "long_rows") *value = h->long_rows;
  else if (k == "long_row_threshold") *value = h->long_row_threshold;
  else if (k == "tail_launches") *value = h->tail_launches;
  else if (k == "plan_bytes") {
    const int64_t vsz = h->value_type == KKAMD_F32 ? 4 : 8, bsz = h->buf_type == KKAMD_F32 ? 4 : 8;
    int64_t b = 0;
    if (h->d_colors) b += 16 * h->nrows + 8 * (h->nrows + 1) + 8 * h->nrows + 4 * h->nnz + 8 * (h->num_colors + 1);
    if (h->d_p_val) b += vsz * (h->nnz + h->nrows);
    if (h->d_X) b += bsz * h->buf_vecs * (h->nrows + h->ncols);
    *value = b;
  } else return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_get: unknown key '%s'", key);
  return KKAMD_OK;
}

int kkamd_gs_export(const kkamd_gs_handle_t* h, const char* what, void* h_out, int64_t count) {
  if (!h || !what) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_export: null argument");
  if (!h->symbolic_complete) return kk::fail(KKAMD_ERR_STATE, "kkamd_gs_export: the symbolic phase has not been completed on this handle");
  const std::string k(what);
  const bool xadj = k == "color_xadj";
  if (!xadj && k != "colors" && k != "color_adj" && k != "old_to_new") return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_export: unknown array '%s'", what);
  const int64_t need = xadj ? h->num_colors + 1 : h->nrows;
  if (count != need) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_export: '%s' has %lld entries, not %lld", what, (long long)need, (long long)count);
  if (need == 0) return KKAMD_OK;
  if (!h_out) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_gs_export: null output");
  int32_t* out = (int32_t*)h_out;
  if (xadj) {
    for (int64_t c = 0; c < need; ++c) out[c] = (int32_t)h->sched.level_off[c];
    return KKAMD_OK;
  }
  const int32_t* src = k == "colors" ? h->d_colors : k == "color_adj" ? h->sched.d_grouped : h->d_old_to_new;
  KK_HIP(hipMemcpy(out, src, sizeof(int32_t) * (size_t)need, hipMemcpyDeviceToHost));
  return KKAMD_OK;
}

}  // extern "C"
