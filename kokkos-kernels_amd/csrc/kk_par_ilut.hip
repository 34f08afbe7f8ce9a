// kk_par_ilut.hip -- threshold incomplete LU by fixed-point iteration: KokkosSparse::Experimental::par_ilut_symbolic / par_ilut_numeric
// (sparse/src/KokkosSparse_par_ilut.hpp, handle sparse/src/KokkosSparse_par_ilut_handle.hpp) for a square, column-sorted CrsMatrix.
//
// Symbolic (sparse/impl/KokkosSparse_par_ilut_symbolic_impl.hpp:36-93): row i of L gets 1 + #{col < i} entries, row i of U 1 + #{col > i};
// both row maps are scanned; nnzL, nnzU and nrows go to the handle.  The graph of A is validated on the host before anything is indexed.
//
// Numeric (sparse/impl/KokkosSparse_par_ilut_numeric_impl.hpp:724-876), the reference's loop step for step; every step is a flat pass with a
// group of LPR lanes per row (a power of two, 1..64; "lanes_per_row", 0 = what covers the mean row of A):
//   product         LU = L * U: the pattern through the library's SpGEMM (kkamd_spgemm_symbolic / _numeric on a handle this one owns), rows
//                   sorted; the values by a kernel of this unit, every entry the sum of its products in ascending k by one lane (the
//                   SpGEMM adds the products of rows of more than 256 entries with floating-point atomics, in the order they arrive);
//   add_candidates  (:129-328) count, scan, fill.  The union of A's row and LU's row by ascending column: an entry of A sits at its index in
//                   A's row plus the entries of LU before it that A lacks; an entry of LU that A lacks at its lower bound in A's row plus
//                   the same count.  That count is an exclusive prefix over LU's row written by the count kernel (one int32 per entry
//                   of LU and one per row).  Old values of L and U are found by bisection;
//   transpose       Ut = U^T through kkamd_transpose, rows sorted;
//   sweep           compute_l_u_factors with async_update == false (:354-458).  The L part of the row is staged in LDS (rows of more than
//                   kPiStage * LPR off-diagonals work in global memory); its entries are a dependent chain in ascending column order:
//                   for each one the lanes stride Ut's row, bisect the L prefix and reduce in a fixed butterfly.  Then every lane takes
//                   U entries of the row and walks Ut's row for each in ascending order, alone;
//   select          (:480-494) radix select over the bit patterns of |v|, 8 bits a pass, LDS histograms of 256 counters added into the
//                   device state with integer atomics; the threshold stays on the device.  The result is the order statistic, exactly;
//   filter          (:496-597) count, scan, fill, stored order kept;
//   residual        (:602-668) one kernel over A's rows that bisects LU's row, per-row partial sums, then one workgroup adds them in a
//                   fixed order; sqrt and the stop test run on the host.
// No floating-point atomics anywhere in this file, and no value of the SpGEMM's is used.  The bits of the factors depend on the lane count in use
// (the L chain's dot products and the residual's row sums are reduced across the group) and on nothing else: the same bits on every run, whatever
// the length of a row of L * U.  NaN values give an unspecified pattern (std::nth_element on NaN is undefined in the
// reference too).
//
// Not here: async_update == true (recorded, without effect, as in the reference: :740), BSR, complex scalars, the reference-side TPL binding.
#include "kk_scan.h"
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <iostream>
#include <limits>
#include <new>
#include <vector>

// Orders one lane group's memory operations between two steps of a row (LDS or global memory), at workgroup scope around the wave barrier;
// nothing relies on the lanes of a wavefront running in lock step.
#ifdef KK_EMU
#define KK_PI_SYNC() kk_emu::sync_wave()
#else
#define KK_PI_SYNC()                                        \
  do {                                                      \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  \
    __builtin_amdgcn_wave_barrier();                        \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");  \
  } while (0)
#endif

namespace kk {

constexpr int kPiStage     = 8;                  // LDS entries of the L part per lane
constexpr int kPiSelShare  = kBlock * 8;         // values per workgroup of a histogram pass before it strides
constexpr int kPiSelBlocks = 1024;

// first index of the ascending list col[0 .. len) whose column is >= c
__device__ __forceinline__ int pi_lower_bound(const int32_t* col, int len, int32_t c) {
  int lo = 0, hi = len;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (col[mid] < c) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int pi_find(const int32_t* col, int len, int32_t c) {
  const int lo = pi_lower_bound(col, len, c);
  return (lo < len && col[lo] == c) ? lo : -1;
}
__device__ __forceinline__ int pi_wave_max(int v) {
  for (int o = kWave >> 1; o > 0; o >>= 1) { const int t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
  return v;
}
// exclusive prefix of v over the aligned group of lpr lanes, the group's sum in *total; every lane of the wavefront calls it
__device__ __forceinline__ int pi_group_scan(int v, int lane, int lpr, int* total) {
  int inc = v;
  for (int o = 1; o < lpr; o <<= 1) {
    const int nb = __shfl_up(inc, (unsigned)o, lpr);
    if (lane >= o) inc += nb;
  }
  *total = __shfl(inc, lpr - 1, lpr);
  return inc - v;
}
template <class VT> __device__ __forceinline__ VT pi_abs(VT v) { return v < VT(0) ? -v : v; }

template <class VT> struct pi_key;
template <> struct pi_key<double> {
  typedef unsigned long long type;
  static constexpr int bits = 64;
  __device__ static type of(double v) { return (type)__double_as_longlong(v) & 0x7fffffffffffffffull; }
  __device__ static double value(type k) { return __longlong_as_double((long long)k); }
};
template <> struct pi_key<float> {
  typedef unsigned long long type;
  static constexpr int bits = 32;
  __device__ static type of(float v) { return (type)((unsigned)__float_as_int(v) & 0x7fffffffu); }
  __device__ static float value(type k) { return __int_as_float((int)(unsigned)k); }
};

// ---------------------------------------------------------------- symbolic and the initial factors
template <class OffT>
__global__ __launch_bounds__(kBlock) void pi_symbolic_kernel(int64_t n, int lpr, int sh, const OffT* __restrict__ A_rm, const int32_t* __restrict__ A_ent,
                                                             OffT* __restrict__ L_rm, OffT* __restrict__ U_rm) {
  const int64_t g = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> sh;
  const int lane = threadIdx.x & (lpr - 1);
  int lo = 0, up = 0;
  if (g < n) {
    const int64_t ae = (int64_t)A_rm[g + 1];
    for (int64_t p = (int64_t)A_rm[g] + lane; p < ae; p += lpr) {
      const int32_t c = A_ent[p];
      lo += c < g; up += c > g;
    }
  }
  lo = group_sum(lo, lpr); up = group_sum(up, lpr);
  if (lane == 0 && g <= n) { L_rm[g] = g < n ? (OffT)(1 + lo) : OffT(0); U_rm[g] = g < n ? (OffT)(1 + up) : OffT(0); }
}

// initialize_LU (:673-719): the strict lower part and a unit diagonal last; the diagonal (1 when A has none) first and the strict upper part.
// A's row is ascending, so an entry's place follows from its index in the row.
template <class OffT, class VT>
__global__ __launch_bounds__(kBlock) void pi_init_kernel(int64_t n, int lpr, int sh, const OffT* __restrict__ A_rm, const int32_t* __restrict__ A_ent,
                                                         const VT* __restrict__ A_val, const OffT* __restrict__ L_rm, int32_t* __restrict__ L_ent,
                                                         VT* __restrict__ L_val, const OffT* __restrict__ U_rm, int32_t* __restrict__ U_ent,
                                                         VT* __restrict__ U_val) {
  const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> sh;
  const int lane = threadIdx.x & (lpr - 1);
  if (row >= n) return;
  const int64_t ab = (int64_t)A_rm[row], ls = (int64_t)L_rm[row], us = (int64_t)U_rm[row];
  const int alen = (int)((int64_t)A_rm[row + 1] - ab), nl = (int)((int64_t)L_rm[row + 1] - ls) - 1, nu = (int)((int64_t)U_rm[row + 1] - us) - 1;
  const int hasdiag = alen - nl - nu;
  if (lane == 0) {
    L_ent[ls + nl] = (int32_t)row; L_val[ls + nl] = VT(1);
    U_ent[us] = (int32_t)row;
    if (!hasdiag) U_val[us] = VT(1);
  }
  for (int j = lane; j < alen; j += lpr) {
    const int32_t c = A_ent[ab + j];
    const VT v = A_val[ab + j];
    if (c < row) { L_ent[ls + j] = c; L_val[ls + j] = v; }
    else if (c == row) U_val[us] = v;
    else { const int64_t k = us + 1 + (j - nl - hasdiag); U_ent[k] = c; U_val[k] = v; }
  }
}

// ---------------------------------------------------------------- add_candidates
// pre: row r owns the int32 entries [LU_rm[r] + r, LU_rm[r + 1] + r + 1): pre[q] = entries of LU's row before q that A's row lacks, and
// the last one their total
template <class OffT>
__global__ __launch_bounds__(kBlock) void pi_cand_count_kernel(int64_t n, int lpr, int sh, const OffT* __restrict__ A_rm, const int32_t* __restrict__ A_ent,
                                                               const OffT* __restrict__ LU_rm, const int32_t* __restrict__ LU_ent,
                                                               OffT* __restrict__ Ln_rm, OffT* __restrict__ Un_rm, int32_t* __restrict__ pre) {
  const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> sh;
  const int lane = threadIdx.x & (lpr - 1);
  const bool valid = row < n;
  int64_t ab = 0, lb = 0;
  int alen = 0, llen = 0;
  if (valid) {
    ab = (int64_t)A_rm[row]; alen = (int)((int64_t)A_rm[row + 1] - ab);
    lb = (int64_t)LU_rm[row]; llen = (int)((int64_t)LU_rm[row + 1] - lb);
  }
  int cl = 0, cu = 0;
  for (int j = lane; j < alen; j += lpr) {
    const int32_t c = A_ent[ab + j];
    cl += c <= row; cu += c >= row;
  }
  int32_t* mypre = pre + lb + row;
  const int trips = pi_wave_max((llen + lpr - 1) / lpr);       // uniform: every lane of the wavefront reaches every shuffle
  int carry = 0;
  for (int it = 0; it < trips; ++it) {
    const int q = it * lpr + lane;
    const bool act = q < llen;
    int f = 0;
    if (act) {
      const int32_t c = LU_ent[lb + q];
      f = pi_find(A_ent + ab, alen, c) < 0;
      if (f) { cl += c <= row; cu += c >= row; }
    }
    int tot;
    const int ex = pi_group_scan(f, lane, lpr, &tot);
    if (act) mypre[q] = carry + ex;
    carry += tot;
  }
  if (valid && lane == 0) mypre[llen] = carry;
  cl = group_sum(cl, lpr); cu = group_sum(cu, lpr);
  if (lane == 0 && row <= n) { Ln_rm[row] = valid ? (OffT)cl : OffT(0); Un_rm[row] = valid ? (OffT)cu : OffT(0); }
}

template <class OffT, class VT>
__global__ __launch_bounds__(kBlock) void pi_cand_fill_kernel(int64_t n, int lpr, int sh, const OffT* __restrict__ A_rm, const int32_t* __restrict__ A_ent,
                                                              const VT* __restrict__ A_val, const OffT* __restrict__ L_rm, const int32_t* __restrict__ L_ent,
                                                              const VT* __restrict__ L_val, const OffT* __restrict__ U_rm, const int32_t* __restrict__ U_ent,
                                                              const VT* __restrict__ U_val, const OffT* __restrict__ LU_rm,
                                                              const int32_t* __restrict__ LU_ent, const VT* __restrict__ LU_val,
                                                              const int32_t* __restrict__ pre, const OffT* __restrict__ Ln_rm, int32_t* __restrict__ Ln_ent,
                                                              VT* __restrict__ Ln_val, const OffT* __restrict__ Un_rm, int32_t* __restrict__ Un_ent,
                                                              VT* __restrict__ Un_val) {
  const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> sh;
  const int lane = threadIdx.x & (lpr - 1);
  if (row >= n) return;
  const int64_t ab = (int64_t)A_rm[row], lb = (int64_t)LU_rm[row], lnb = (int64_t)Ln_rm[row], unb = (int64_t)Un_rm[row];
  const int alen = (int)((int64_t)A_rm[row + 1] - ab), llen = (int)((int64_t)LU_rm[row + 1] - lb);
  const int cu = (int)((int64_t)Un_rm[row + 1] - unb);
  const int64_t lob = (int64_t)L_rm[row], uob = (int64_t)U_rm[row];
  const int lon = (int)((int64_t)L_rm[row + 1] - lob) - 1, uon = (int)((int64_t)U_rm[row + 1] - uob);   // the old L's diagonal is skipped
  const int32_t* mypre = pre + lb + row;
  const int below = alen + mypre[llen] - cu;                  // columns of the union before the first one >= row
  for (int pass = 0; pass < 2; ++pass) {
    const int len = pass == 0 ? alen : llen;
    for (int j = lane; j < len; j += lpr) {
      int32_t c; VT a = VT(0), lu = VT(0);
      int rank;
      if (pass == 0) {
        c = A_ent[ab + j]; a = A_val[ab + j];
        const int q = pi_lower_bound(LU_ent + lb, llen, c);
        if (q < llen && LU_ent[lb + q] == c) lu = LU_val[lb + q];
        rank = j + mypre[q];
      } else {
        c = LU_ent[lb + j];
        const int p = pi_lower_bound(A_ent + ab, alen, c);
        if (p < alen && A_ent[ab + p] == c) continue;          // A's pass took it
        lu = LU_val[lb + j];
        rank = p + mypre[j];
      }
      const VT r = a - lu;
      VT out;
      if (c < row) {
        const int pos = pi_find(L_ent + lob, lon, c);
        out = pos >= 0 ? L_val[lob + pos] : r / U_val[(int64_t)U_rm[c]];    // the diagonal is first in a row of U
      } else {
        const int pos = pi_find(U_ent + uob, uon, c);
        out = pos >= 0 ? U_val[uob + pos] : r;
      }
      if (c <= row) { Ln_ent[lnb + rank] = c; Ln_val[lnb + rank] = c == row ? VT(1) : out; }
      if (c >= row) { Un_ent[unb + (rank - below)] = c; Un_val[unb + (rank - below)] = out; }
    }
  }
}

// ---------------------------------------------------------------- the sweep
// L_val and U_val are renewed in place: neither const nor __restrict__.  Ut is frozen for the whole launch.
template <class OffT, class VT>
__global__ __launch_bounds__(kBlock) void pi_sweep_kernel(int64_t n, int lpr, int sh, const OffT* __restrict__ A_rm, const int32_t* __restrict__ A_ent,
                                                          const VT* __restrict__ A_val, const OffT* __restrict__ L_rm, const int32_t* __restrict__ L_ent,
                                                          VT* L_val, const OffT* __restrict__ U_rm, const int32_t* __restrict__ U_ent, VT* U_val,
                                                          const OffT* __restrict__ Ut_rm, const int32_t* __restrict__ Ut_ent,
                                                          const VT* __restrict__ Ut_val) {
  __shared__ int32_t s_col[kBlock * kPiStage];
  __shared__ VT s_val[kBlock * kPiStage];
  const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> sh;
  const int lane = threadIdx.x & (lpr - 1);
  const int slice = ((int)threadIdx.x >> sh) * lpr * kPiStage;
  const bool valid = row < n;
  int64_t ls = 0, ab = 0;
  int np = 0, alen = 0;                                        // np: the off-diagonals of the L row (its diagonal is last)
  if (valid) {
    ls = (int64_t)L_rm[row]; np = (int)((int64_t)L_rm[row + 1] - ls) - 1;
    if (np < 0) np = 0;
    ab = (int64_t)A_rm[row]; alen = (int)((int64_t)A_rm[row + 1] - ab);
  }
  const bool staged = valid && np <= kPiStage * lpr;
  const int32_t* lc = L_ent + ls;
  VT* lv = L_val + ls;
  if (staged) {
    for (int j = lane; j < np; j += lpr) { s_col[slice + j] = L_ent[ls + j]; s_val[slice + j] = L_val[ls + j]; }
    lc = s_col + slice; lv = s_val + slice;
  }
  KK_PI_SYNC();
  const int maxp = pi_wave_max(np);
  for (int t = 0; t < maxp; ++t) {
    const bool act = t < np;
    VT part = VT(0), udiag = VT(0);
    int32_t c = 0;
    if (act) {
      c = lc[t];
      const int64_t tb = (int64_t)Ut_rm[c], te = (int64_t)Ut_rm[c + 1];
      udiag = te > tb ? Ut_val[te - 1] : VT(0);              // U(c, c) is last in row c of Ut
      if (udiag != VT(0))
        for (int64_t p = tb + lane; p < te; p += lpr) {
          const int32_t k = Ut_ent[p];
          if (k >= c) break;                                   // k < min(row, c) = c
          const int pos = pi_find(lc, t, k);                   // the columns of this row's L before c
          if (pos >= 0) part = part + lv[pos] * Ut_val[p];
        }
    }
    const VT sum = group_sum(part, lpr);
    if (act && lane == 0 && udiag != VT(0)) {
      const int pa = pi_find(A_ent + ab, alen, c);
      const VT a = pa >= 0 ? A_val[ab + pa] : VT(0);
      lv[t] = (a - sum) / udiag;
    }
    KK_PI_SYNC();                                              // the next entry reads this one
  }
  if (valid) {
    const int64_t us = (int64_t)U_rm[row];
    const int nu = (int)((int64_t)U_rm[row + 1] - us);
    for (int t = lane; t < nu; t += lpr) {
      const int32_t c = U_ent[us + t];
      const int64_t te = (int64_t)Ut_rm[c + 1];
      VT sum = VT(0);
      for (int64_t p = (int64_t)Ut_rm[c]; p < te; ++p) {
        const int32_t k = Ut_ent[p];
        if (k >= row) break;                                   // k < min(row, c) = row
        const int pos = pi_find(lc, np, k);
        if (pos >= 0) sum = sum + lv[pos] * Ut_val[p];
      }
      const int pa = pi_find(A_ent + ab, alen, c);
      const VT a = pa >= 0 ? A_val[ab + pa] : VT(0);
      U_val[us + t] = a - sum;
    }
  }
  KK_PI_SYNC();
  if (staged)
    for (int j = lane; j < np; j += lpr) L_val[ls + j] = s_val[slice + j];
}

// ---------------------------------------------------------------- select
struct PiSelState {
  unsigned long long prefix, rank;
  unsigned long long hist[256];
};
__global__ void pi_sel_init_kernel(PiSelState* s, unsigned long long rank) {
  for (int t = threadIdx.x; t < 256; t += blockDim.x) s->hist[t] = 0ull;
  if (threadIdx.x == 0) { s->prefix = 0ull; s->rank = rank; }
}
// counts, by the 8 bits at `shift`, the values whose key agrees with the prefix above those bits
template <class VT>
__global__ __launch_bounds__(kBlock) void pi_sel_hist_kernel(const VT* __restrict__ v, int64_t n, int shift, int first, PiSelState* s) {
  __shared__ unsigned s_hist[256];
  s_hist[threadIdx.x] = 0u;                                  // kBlock == 256
  __syncthreads();
  const unsigned long long prefix = s->prefix;
  const int hs = shift + 8;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const unsigned long long key = pi_key<VT>::of(v[i]);
    if (first || (key >> hs) == (prefix >> hs)) atomicAdd(&s_hist[(unsigned)(key >> shift) & 255u], 1u);
  }
  __syncthreads();
  const unsigned cnt = s_hist[threadIdx.x];
  if (cnt) atomicAdd(&s->hist[threadIdx.x], (unsigned long long)cnt);
}
template <class VT>
__global__ void pi_sel_pick_kernel(PiSelState* s, int shift, int last, VT* out) {
  if (threadIdx.x != 0) return;
  unsigned long long r = s->rank;
  int b = 0;
  for (; b < 255; ++b) {
    const unsigned long long cnt = s->hist[b];
    if (r < cnt) break;
    r -= cnt;
  }
  s->prefix |= (unsigned long long)b << shift;
  s->rank = r;
  for (int t = 0; t < 256; ++t) s->hist[t] = 0ull;
  if (last) *out = pi_key<VT>::value(s->prefix);
}

// ---------------------------------------------------------------- filter
template <class OffT, class VT>
__global__ __launch_bounds__(kBlock) void pi_filter_count_kernel(int64_t n, int lpr, int sh, const OffT* __restrict__ I_rm, const int32_t* __restrict__ I_ent,
                                                                 const VT* __restrict__ I_val, const VT* __restrict__ thr, OffT* __restrict__ O_rm) {
  const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> sh;
  const int lane = threadIdx.x & (lpr - 1);
  const VT th = *thr;
  int cnt = 0;
  if (row < n) {
    const int64_t ie = (int64_t)I_rm[row + 1];
    for (int64_t p = (int64_t)I_rm[row] + lane; p < ie; p += lpr) cnt += (pi_abs(I_val[p]) >= th || I_ent[p] == row) ? 1 : 0;
  }
  cnt = group_sum(cnt, lpr);
  if (lane == 0 && row <= n) O_rm[row] = row < n ? (OffT)cnt : OffT(0);
}
template <class OffT, class VT>
__global__ __launch_bounds__(kBlock) void pi_filter_fill_kernel(int64_t n, int lpr, int sh, const OffT* __restrict__ I_rm, const int32_t* __restrict__ I_ent,
                                                                const VT* __restrict__ I_val, const VT* __restrict__ thr, const OffT* __restrict__ O_rm,
                                                                int32_t* __restrict__ O_ent, VT* __restrict__ O_val) {
  const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> sh;
  const int lane = threadIdx.x & (lpr - 1);
  const VT th = *thr;
  int64_t ib = 0, ob = 0;
  int len = 0;
  if (row < n) { ib = (int64_t)I_rm[row]; len = (int)((int64_t)I_rm[row + 1] - ib); ob = (int64_t)O_rm[row]; }
  const int trips = pi_wave_max((len + lpr - 1) / lpr);
  int carry = 0;
  for (int it = 0; it < trips; ++it) {
    const int q = it * lpr + lane;
    int keep = 0;
    int32_t c = 0;
    VT v = VT(0);
    if (q < len) { c = I_ent[ib + q]; v = I_val[ib + q]; keep = (pi_abs(v) >= th || c == row) ? 1 : 0; }
    int tot;
    const int ex = pi_group_scan(keep, lane, lpr, &tot);
    if (keep) { O_ent[ob + carry + ex] = c; O_val[ob + carry + ex] = v; }
    carry += tot;
  }
}

// ---------------------------------------------------------------- the product's values
// LU(row, c) = sum over the entries k of L's row, ascending, of L(row, k) * U(k, c), one lane per entry of LU's row: a fixed order, the same
// under every lane count.  U's row k is bisected for c (it holds no column below k).
template <class OffT, class VT>
__global__ __launch_bounds__(kBlock) void pi_product_values_kernel(int64_t n, int lpr, int sh, const OffT* __restrict__ L_rm, const int32_t* __restrict__ L_ent,
                                                                   const VT* __restrict__ L_val, const OffT* __restrict__ U_rm,
                                                                   const int32_t* __restrict__ U_ent, const VT* __restrict__ U_val,
                                                                   const OffT* __restrict__ LU_rm, const int32_t* __restrict__ LU_ent,
                                                                   VT* __restrict__ LU_val) {
  const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> sh;
  const int lane = threadIdx.x & (lpr - 1);
  if (row >= n) return;
  const int64_t ls = (int64_t)L_rm[row], pe = (int64_t)LU_rm[row + 1];
  const int nl = (int)((int64_t)L_rm[row + 1] - ls);
  for (int64_t p = (int64_t)LU_rm[row] + lane; p < pe; p += lpr) {
    const int32_t c = LU_ent[p];
    VT s = VT(0);
    for (int j = 0; j < nl; ++j) {
      const int32_t k = L_ent[ls + j];
      if (k > c) break;                                        // U(k, c) needs k <= c, and L's row ascends
      const int64_t ub = (int64_t)U_rm[k];
      const int pos = pi_find(U_ent + ub, (int)((int64_t)U_rm[k + 1] - ub), c);
      if (pos >= 0) s = s + L_val[ls + j] * U_val[ub + pos];
    }
    LU_val[p] = s;
  }
}

// ---------------------------------------------------------------- residual
template <class OffT, class VT>
__global__ __launch_bounds__(kBlock) void pi_resid_rows_kernel(int64_t n, int lpr, int sh, const OffT* __restrict__ A_rm, const int32_t* __restrict__ A_ent,
                                                               const VT* __restrict__ A_val, const OffT* __restrict__ LU_rm,
                                                               const int32_t* __restrict__ LU_ent, const VT* __restrict__ LU_val, VT* __restrict__ rowsum) {
  const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> sh;
  const int lane = threadIdx.x & (lpr - 1);
  VT part = VT(0);
  if (row < n) {
    const int64_t ae = (int64_t)A_rm[row + 1], lb = (int64_t)LU_rm[row];
    const int llen = (int)((int64_t)LU_rm[row + 1] - lb);
    for (int64_t p = (int64_t)A_rm[row] + lane; p < ae; p += lpr) {
      const int pos = pi_find(LU_ent + lb, llen, A_ent[p]);
      const VT d = A_val[p] - (pos >= 0 ? LU_val[lb + pos] : VT(0));
      part = part + d * d;
    }
  }
  part = group_sum(part, lpr);
  if (lane == 0 && row < n) rowsum[row] = part;
}
// one workgroup: thread t adds rows t, t + 256, ... in ascending order, then a fixed tree
template <class VT>
__global__ __launch_bounds__(kBlock) void pi_resid_reduce_kernel(const VT* __restrict__ rowsum, int64_t n, VT* __restrict__ out) {
  __shared__ VT s_part[kBlock];
  VT acc = VT(0);
  for (int64_t i = threadIdx.x; i < n; i += kBlock) acc = acc + rowsum[i];
  s_part[threadIdx.x] = acc;
  __syncthreads();
  for (int o = kBlock >> 1; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s_part[threadIdx.x] = s_part[threadIdx.x] + s_part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = s_part[0];
}

// a device buffer of the handle: it only grows
struct PiBuf {
  void* p = nullptr;
  size_t cap = 0;
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};
struct PiCsr { PiBuf rm, ent, val; int64_t nnz = 0; };

}  // namespace kk

struct kkamd_par_ilut_handle {
  // the reference's inputs (sparse/src/KokkosKernels_Handle.hpp:871-881) and the library's knob
  int64_t max_iter = 20;
  double residual_norm_delta_stop = 1e-2, fill_in_limit = 0.75;
  int async_update = 0, verbose = 0, lanes_per_row = 0, profile = 0;
  double step_ms[7] = {0, 0, 0, 0, 0, 0, 0};                // "profile": product, candidates, transpose, sweep, select, filter, residual
  // symbolic
  int64_t nrows = 0, nnzA = 0, nnzL = 0, nnzU = 0;
  int offset_type = -1;
  bool symbolic_complete = false, numeric_complete = false;
  kk::PiBuf sym_L_rm, sym_U_rm;                             // numeric overwrites the caller's row maps with the final ones
  // numeric
  int value_type = -1;
  int64_t num_iters = -1, host_syncs = 0, launches = 0, max_product_row = 0;
  double end_rel_res = -1, l_threshold = 0, u_threshold = 0;
  kkamd_spgemm_handle_t* spgemm = nullptr;
  kk::PiCsr L, U, Ln, Un, Ut, LU;
  kk::PiBuf pre, scanws, rowsum, sel, scal;                 // scal: the two thresholds and the residual's sum, of the value type
  int64_t bytes = 0;
};

namespace kk {

static int pi_ensure(kkamd_par_ilut_handle* h, PiBuf* b, size_t bytes) {
  if (bytes <= b->cap && b->p) return KKAMD_OK;
  if (b->p) { (void)hipFree(b->p); b->p = nullptr; h->bytes -= (int64_t)b->cap; b->cap = 0; }
  const size_t want = bytes ? bytes : 16;
  if (hipMalloc(&b->p, want) != hipSuccess) { b->p = nullptr; return fail(KKAMD_ERR_ALLOC, "kkamd_par_ilut: out of device memory (%zu bytes)", want); }
  b->cap = want; h->bytes += (int64_t)want;
  return KKAMD_OK;
}
static void pi_free(kkamd_par_ilut_handle* h, PiBuf* b) {
  if (b->p) { (void)hipFree(b->p); h->bytes -= (int64_t)b->cap; }
  b->p = nullptr; b->cap = 0;
}
static int pi_ensure_csr(kkamd_par_ilut_handle* h, PiCsr* m, int64_t nnz, size_t vsz) {
  int rc = pi_ensure(h, &m->ent, sizeof(int32_t) * (size_t)nnz);
  if (rc == KKAMD_OK) rc = pi_ensure(h, &m->val, vsz * (size_t)nnz);
  return rc;
}
#define KK_PI(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

static int pi_log2(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }
static int pi_lanes(const kkamd_par_ilut_handle* h, int64_t n, int64_t nnzA) {
  if (h->lanes_per_row) return h->lanes_per_row;
  const int64_t mean = n > 0 ? ceil_div(nnzA, n) : 1;
  int lpr = 1;
  while (lpr < kWave && lpr < mean) lpr *= 2;
  return lpr;
}
static unsigned pi_grid(int64_t groups, int lpr) { return (unsigned)std::max<int64_t>(1, ceil_div(groups * lpr, kBlock)); }
// launches of one exclusive_scan_inplace over n items
static int pi_scan_launches(int64_t n) { int c = 0; while (n > kScanTile) { n = ceil_div(n, kScanTile); c += 2; } return c + 1; }

template <class OffT>
static int pi_scan(kkamd_par_ilut_handle* h, OffT* d, int64_t n, hipStream_t st) {
  KK_PI(pi_ensure(h, &h->scanws, sizeof(int64_t) * (size_t)scan_workspace_items(n)));
  h->launches += pi_scan_launches(n);
  return exclusive_scan_inplace<OffT>(d, n, st, h->scanws.as<OffT>());
}
template <class OffT>
static int pi_read_totals(kkamd_par_ilut_handle* h, const OffT* a_rm, const OffT* b_rm, int64_t n, int64_t* a, int64_t* b, hipStream_t st) {
  OffT t[2] = {0, 0};
  KK_HIP(hipMemcpyAsync(&t[0], a_rm + n, sizeof(OffT), hipMemcpyDeviceToHost, st));
  if (b_rm) KK_HIP(hipMemcpyAsync(&t[1], b_rm + n, sizeof(OffT), hipMemcpyDeviceToHost, st));
  KK_HIP(hipStreamSynchronize(st));
  ++h->host_syncs;
  *a = (int64_t)t[0];
  if (b) *b = (int64_t)t[1];
  return KKAMD_OK;
}

// ---- the steps on device arrays; the entry points below and the loop share them
template <class OffT, class VT>
static int pi_candidates_count(kkamd_par_ilut_handle* h, int64_t n, int lpr, const OffT* A_rm, const int32_t* A_ent, const OffT* LU_rm, const int32_t* LU_ent,
                               int64_t nnzLU, int64_t nnzA, OffT* Ln_rm, OffT* Un_rm, int64_t* nnzLn, int64_t* nnzUn, hipStream_t st) {
  if (nnzA < 0) KK_PI(pi_read_totals<OffT>(h, A_rm, (const OffT*)nullptr, n, &nnzA, nullptr, st));   // the step entry point: A's size is on the device
  // neither union exceeds nnz(A) + nnz(LU); with 32-bit offsets a larger bound could wrap inside the scans
  if (sizeof(OffT) == 4 && nnzA + nnzLU > (int64_t)INT32_MAX)
    return fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut: the candidates of L or U may have more than 2^31 - 1 entries (nnz(A) %lld + nnz(L U) %lld): use 64-bit offsets",
                (long long)nnzA, (long long)nnzLU);
  KK_PI(pi_ensure(h, &h->pre, sizeof(int32_t) * (size_t)(nnzLU + n + 1)));
  KK_LAUNCH((pi_cand_count_kernel<OffT>), pi_grid(n + 1, lpr), kBlock, 0, st, n, lpr, pi_log2(lpr), A_rm, A_ent, LU_rm, LU_ent, Ln_rm, Un_rm, h->pre.as<int32_t>());
  ++h->launches;
  KK_PI(pi_scan<OffT>(h, Ln_rm, n + 1, st));
  KK_PI(pi_scan<OffT>(h, Un_rm, n + 1, st));
  KK_LAUNCH_CHECK();
  return pi_read_totals<OffT>(h, Ln_rm, Un_rm, n, nnzLn, nnzUn, st);
}
template <class OffT, class VT>
static int pi_candidates_fill(kkamd_par_ilut_handle* h, int64_t n, int lpr, const OffT* A_rm, const int32_t* A_ent, const VT* A_val, const OffT* L_rm,
                              const int32_t* L_ent, const VT* L_val, const OffT* U_rm, const int32_t* U_ent, const VT* U_val, const OffT* LU_rm,
                              const int32_t* LU_ent, const VT* LU_val, const OffT* Ln_rm, int32_t* Ln_ent, VT* Ln_val, const OffT* Un_rm, int32_t* Un_ent,
                              VT* Un_val, hipStream_t st) {
  KK_LAUNCH((pi_cand_fill_kernel<OffT, VT>), pi_grid(n, lpr), kBlock, 0, st, n, lpr, pi_log2(lpr), A_rm, A_ent, A_val, L_rm, L_ent, L_val, U_rm, U_ent, U_val,
            LU_rm, LU_ent, LU_val, (const int32_t*)h->pre.as<int32_t>(), Ln_rm, Ln_ent, Ln_val, Un_rm, Un_ent, Un_val);
  ++h->launches;
  KK_LAUNCH_CHECK();
  return KKAMD_OK;
}
template <class OffT, class VT>
static int pi_sweep(kkamd_par_ilut_handle* h, int64_t n, int lpr, const OffT* A_rm, const int32_t* A_ent, const VT* A_val, const OffT* L_rm,
                    const int32_t* L_ent, VT* L_val, const OffT* U_rm, const int32_t* U_ent, VT* U_val, const OffT* Ut_rm, const int32_t* Ut_ent,
                    const VT* Ut_val, hipStream_t st) {
  KK_LAUNCH((pi_sweep_kernel<OffT, VT>), pi_grid(n, lpr), kBlock, 0, st, n, lpr, pi_log2(lpr), A_rm, A_ent, A_val, L_rm, L_ent, L_val, U_rm, U_ent, U_val, Ut_rm,
            Ut_ent, Ut_val);
  ++h->launches;
  KK_LAUNCH_CHECK();
  return KKAMD_OK;
}
template <class VT>
static int pi_select(kkamd_par_ilut_handle* h, const VT* v, int64_t cnt, int64_t rank, VT* d_out, hipStream_t st) {
  KK_PI(pi_ensure(h, &h->sel, sizeof(PiSelState)));
  PiSelState* s = h->sel.as<PiSelState>();
  KK_LAUNCH(pi_sel_init_kernel, 1u, kBlock, 0, st, s, (unsigned long long)rank);
  const unsigned grid = (unsigned)std::min<int64_t>(kPiSelBlocks, std::max<int64_t>(1, ceil_div(cnt, kPiSelShare)));
  for (int shift = pi_key<VT>::bits - 8; shift >= 0; shift -= 8) {
    KK_LAUNCH((pi_sel_hist_kernel<VT>), grid, kBlock, 0, st, v, cnt, shift, shift == pi_key<VT>::bits - 8 ? 1 : 0, s);
    KK_LAUNCH((pi_sel_pick_kernel<VT>), 1u, kWave, 0, st, s, shift, shift == 0 ? 1 : 0, d_out);
    h->launches += 2;
  }
  ++h->launches;
  KK_LAUNCH_CHECK();
  return KKAMD_OK;
}
template <class OffT, class VT>
static int pi_filter_count(kkamd_par_ilut_handle* h, int64_t n, int lpr, const OffT* I_rm, const int32_t* I_ent, const VT* I_val, const VT* thr, OffT* O_rm,
                           hipStream_t st) {
  KK_LAUNCH((pi_filter_count_kernel<OffT, VT>), pi_grid(n + 1, lpr), kBlock, 0, st, n, lpr, pi_log2(lpr), I_rm, I_ent, I_val, thr, O_rm);
  ++h->launches;
  return pi_scan<OffT>(h, O_rm, n + 1, st);
}
template <class OffT, class VT>
static int pi_filter_fill(kkamd_par_ilut_handle* h, int64_t n, int lpr, const OffT* I_rm, const int32_t* I_ent, const VT* I_val, const VT* thr, const OffT* O_rm,
                          int32_t* O_ent, VT* O_val, hipStream_t st) {
  KK_LAUNCH((pi_filter_fill_kernel<OffT, VT>), pi_grid(n, lpr), kBlock, 0, st, n, lpr, pi_log2(lpr), I_rm, I_ent, I_val, thr, O_rm, O_ent, O_val);
  ++h->launches;
  KK_LAUNCH_CHECK();
  return KKAMD_OK;
}
// the sum of squares into d_out, on the stream
template <class OffT, class VT>
static int pi_residual(kkamd_par_ilut_handle* h, int64_t n, int lpr, const OffT* A_rm, const int32_t* A_ent, const VT* A_val, const OffT* LU_rm,
                       const int32_t* LU_ent, const VT* LU_val, VT* d_out, hipStream_t st) {
  KK_PI(pi_ensure(h, &h->rowsum, sizeof(VT) * (size_t)n));
  KK_LAUNCH((pi_resid_rows_kernel<OffT, VT>), pi_grid(n, lpr), kBlock, 0, st, n, lpr, pi_log2(lpr), A_rm, A_ent, A_val, LU_rm, LU_ent, LU_val, h->rowsum.as<VT>());
  KK_LAUNCH((pi_resid_reduce_kernel<VT>), 1u, kBlock, 0, st, (const VT*)h->rowsum.as<VT>(), n, d_out);
  h->launches += 2;
  KK_LAUNCH_CHECK();
  return KKAMD_OK;
}

// LU = L * U, rows sorted.  The pattern is the SpGEMM's: its symbolic phase sizes the product, its numeric phase writes the sorted entries.
// The SpGEMM handle answers a second symbolic call on the same row map arrays from memory, and these arrays are the same every iteration with
// another pattern in them: "symbolic_computed" 0 makes it analyse again.  The VALUES are then written by pi_product_values_kernel, because
// the SpGEMM adds the products of a row of more than 256 entries with floating-point atomics, in the order they arrive: here every entry is the
// sum of its products in ascending k, so the product has the same bits on every run and under every lane count.
template <class OffT, class VT>
static int pi_product(kkamd_par_ilut_handle* h, int64_t n, int lpr, hipStream_t st) {
  const int off = sizeof(OffT) == 8 ? KKAMD_I64 : KKAMD_I32;
  kkamd_stream_t kst = reinterpret_cast<kkamd_stream_t>(st);
  KK_PI(pi_ensure(h, &h->LU.rm, sizeof(OffT) * (size_t)(n + 1)));
  KK_PI(kkamd_spgemm_set(h->spgemm, "symbolic_computed", 0));
  int64_t c_nnz = 0;
  KK_PI(kkamd_spgemm_symbolic(h->spgemm, n, n, n, h->L.rm.p, h->L.ent.as<int32_t>(), h->U.rm.p, h->U.ent.as<int32_t>(), h->LU.rm.p, off, &c_nnz, kst));
  KK_PI(pi_ensure_csr(h, &h->LU, c_nnz, sizeof(VT)));
  h->LU.nnz = c_nnz;
  int64_t longest = 0;
  KK_PI(kkamd_spgemm_get(h->spgemm, 3, &longest));
  h->max_product_row = std::max(h->max_product_row, longest);
  KK_PI(kkamd_spgemm_set(h->spgemm, "entries_computed", 0));
  KK_PI(kkamd_spgemm_numeric(h->spgemm, n, n, n, h->L.rm.p, h->L.ent.as<int32_t>(), h->L.val.p, h->U.rm.p, h->U.ent.as<int32_t>(), h->U.val.p, h->LU.rm.p,
                             h->LU.ent.as<int32_t>(), h->LU.val.p, off, scalar_tag<VT>::value, kst));
  KK_LAUNCH((pi_product_values_kernel<OffT, VT>), pi_grid(n, lpr), kBlock, 0, st, n, lpr, pi_log2(lpr), (const OffT*)h->L.rm.as<OffT>(),
            (const int32_t*)h->L.ent.as<int32_t>(), (const VT*)h->L.val.as<VT>(), (const OffT*)h->U.rm.as<OffT>(), (const int32_t*)h->U.ent.as<int32_t>(),
            (const VT*)h->U.val.as<VT>(), (const OffT*)h->LU.rm.as<OffT>(), (const int32_t*)h->LU.ent.as<int32_t>(), h->LU.val.as<VT>());
  ++h->launches;
  KK_LAUNCH_CHECK();
  return KKAMD_OK;
}
template <class OffT, class VT>
static int pi_transpose(kkamd_par_ilut_handle* h, int64_t n, const PiCsr& U, hipStream_t st) {
  KK_PI(pi_ensure(h, &h->Ut.rm, sizeof(OffT) * (size_t)(n + 1)));
  KK_PI(pi_ensure_csr(h, &h->Ut, U.nnz, sizeof(VT)));
  h->Ut.nnz = U.nnz;
  return kkamd_transpose(n, n, U.nnz, U.rm.p, U.ent.as<int32_t>(), U.val.p, sizeof(OffT) == 8 ? KKAMD_I64 : KKAMD_I32, scalar_tag<VT>::value, h->Ut.rm.p,
                         h->Ut.ent.as<int32_t>(), h->Ut.val.p, reinterpret_cast<kkamd_stream_t>(st));
}

template <class OffT, class VT>
static int pi_numeric_typed(kkamd_par_ilut_handle* h, int64_t n, const OffT* A_rm, const int32_t* A_ent, const VT* A_val, OffT* L_rm_out, OffT* U_rm_out,
                            hipStream_t st) {
  const int lpr = pi_lanes(h, n, h->nnzA);
  const size_t rmb = sizeof(OffT) * (size_t)(n + 1);
  h->host_syncs = 0; h->launches = 0; h->max_product_row = 0;
  const int64_t limit_L = (int64_t)(h->fill_in_limit * (double)h->nnzL), limit_U = (int64_t)(h->fill_in_limit * (double)h->nnzU);
  const bool do_residual = h->residual_norm_delta_stop > 0;
  if (h->verbose) {
    std::cout << "Starting PARILUT with..." << std::endl;
    std::cout << "  num_rows:            " << n << std::endl;
    std::cout << "  fill_in_limit:       " << h->fill_in_limit << std::endl;
    std::cout << "  max_iter:            " << h->max_iter << std::endl;
    std::cout << "  res_norm_delta_stop: " << h->residual_norm_delta_stop << std::endl;
    std::cout << "  async_update:        " << false << std::endl;
  }
  PiCsr &L = h->L, &U = h->U, &Ln = h->Ln, &Un = h->Un, &Ut = h->Ut, &LU = h->LU;
  for (PiCsr* m : {&L, &U, &Ln, &Un}) KK_PI(pi_ensure(h, &m->rm, rmb));
  KK_PI(pi_ensure(h, &h->scal, 4 * sizeof(VT)));
  VT* d_scal = h->scal.as<VT>();
  KK_HIP(hipMemcpyAsync(L.rm.p, h->sym_L_rm.p, rmb, hipMemcpyDeviceToDevice, st));
  KK_HIP(hipMemcpyAsync(U.rm.p, h->sym_U_rm.p, rmb, hipMemcpyDeviceToDevice, st));
  L.nnz = h->nnzL; U.nnz = h->nnzU;
  KK_PI(pi_ensure_csr(h, &L, L.nnz, sizeof(VT)));
  KK_PI(pi_ensure_csr(h, &U, U.nnz, sizeof(VT)));
  int64_t itr = 0;
  VT curr = std::numeric_limits<VT>::max(), prev = std::numeric_limits<VT>::max();
  if (n > 0) {
    KK_LAUNCH((pi_init_kernel<OffT, VT>), pi_grid(n, lpr), kBlock, 0, st, n, lpr, pi_log2(lpr), A_rm, A_ent, A_val, (const OffT*)L.rm.as<OffT>(), L.ent.as<int32_t>(),
              L.val.as<VT>(), (const OffT*)U.rm.as<OffT>(), U.ent.as<int32_t>(), U.val.as<VT>());
    ++h->launches;
    KK_LAUNCH_CHECK();
  }
  // "profile": the stream is synchronised after every step and the host clock read
  auto t_last = std::chrono::steady_clock::now();
  auto tick = [&](int step) {
    if (!h->profile) return;
    (void)hipStreamSynchronize(st);
    const auto t = std::chrono::steady_clock::now();
    h->step_ms[step] += std::chrono::duration<double, std::milli>(t - t_last).count();
    t_last = t;
  };
  tick(0);
  for (double& t : h->step_ms) t = 0;
  bool stop = n == 0;
  while (!stop && itr < h->max_iter) {
    // 1. the product, unless the residual step of the iteration before left it
    if (itr == 0 || !do_residual) KK_PI((pi_product<OffT, VT>(h, n, lpr, st)));
    tick(0);
    // 2. add_candidates
    KK_PI((pi_candidates_count<OffT, VT>(h, n, lpr, A_rm, A_ent, LU.rm.as<OffT>(), LU.ent.as<int32_t>(), LU.nnz, h->nnzA, Ln.rm.as<OffT>(), Un.rm.as<OffT>(), &Ln.nnz, &Un.nnz, st)));
    KK_PI(pi_ensure_csr(h, &Ln, Ln.nnz, sizeof(VT)));
    KK_PI(pi_ensure_csr(h, &Un, Un.nnz, sizeof(VT)));
    KK_PI((pi_candidates_fill<OffT, VT>(h, n, lpr, A_rm, A_ent, A_val, L.rm.as<OffT>(), L.ent.as<int32_t>(), L.val.as<VT>(), U.rm.as<OffT>(), U.ent.as<int32_t>(),
                                        U.val.as<VT>(), LU.rm.as<OffT>(), LU.ent.as<int32_t>(), LU.val.as<VT>(), Ln.rm.as<OffT>(), Ln.ent.as<int32_t>(),
                                        Ln.val.as<VT>(), Un.rm.as<OffT>(), Un.ent.as<int32_t>(), Un.val.as<VT>(), st)));
    tick(1);
    // 3, 4. the transpose of U_new and the first sweep
    KK_PI((pi_transpose<OffT, VT>(h, n, Un, st)));
    tick(2);
    KK_PI((pi_sweep<OffT, VT>(h, n, lpr, A_rm, A_ent, A_val, Ln.rm.as<OffT>(), Ln.ent.as<int32_t>(), Ln.val.as<VT>(), Un.rm.as<OffT>(), Un.ent.as<int32_t>(),
                              Un.val.as<VT>(), Ut.rm.as<OffT>(), Ut.ent.as<int32_t>(), Ut.val.as<VT>(), st)));
    tick(3);
    // 5. select and filter: the results become L and U
    const int64_t rank_L = std::max<int64_t>(0, Ln.nnz - limit_L - 1), rank_U = std::max<int64_t>(0, Un.nnz - limit_U - 1);
    KK_PI(pi_select<VT>(h, Ln.val.as<VT>(), Ln.nnz, rank_L, d_scal + 0, st));
    KK_PI(pi_select<VT>(h, Un.val.as<VT>(), Un.nnz, rank_U, d_scal + 1, st));
    tick(4);
    KK_PI(pi_ensure_csr(h, &L, Ln.nnz, sizeof(VT)));
    KK_PI(pi_ensure_csr(h, &U, Un.nnz, sizeof(VT)));
    KK_PI((pi_filter_count<OffT, VT>(h, n, lpr, Ln.rm.as<OffT>(), Ln.ent.as<int32_t>(), Ln.val.as<VT>(), d_scal + 0, L.rm.as<OffT>(), st)));
    KK_PI((pi_filter_count<OffT, VT>(h, n, lpr, Un.rm.as<OffT>(), Un.ent.as<int32_t>(), Un.val.as<VT>(), d_scal + 1, U.rm.as<OffT>(), st)));
    KK_PI((pi_filter_fill<OffT, VT>(h, n, lpr, Ln.rm.as<OffT>(), Ln.ent.as<int32_t>(), Ln.val.as<VT>(), d_scal + 0, L.rm.as<OffT>(), L.ent.as<int32_t>(), L.val.as<VT>(), st)));
    KK_PI((pi_filter_fill<OffT, VT>(h, n, lpr, Un.rm.as<OffT>(), Un.ent.as<int32_t>(), Un.val.as<VT>(), d_scal + 1, U.rm.as<OffT>(), U.ent.as<int32_t>(), U.val.as<VT>(), st)));
    VT thr[2];
    KK_HIP(hipMemcpyAsync(thr, d_scal, 2 * sizeof(VT), hipMemcpyDeviceToHost, st));
    KK_PI((pi_read_totals<OffT>(h, L.rm.as<OffT>(), U.rm.as<OffT>(), n, &L.nnz, &U.nnz, st)));
    h->l_threshold = (double)thr[0]; h->u_threshold = (double)thr[1];
    tick(5);
    // 6. the transpose of U and the second sweep
    KK_PI((pi_transpose<OffT, VT>(h, n, U, st)));
    tick(2);
    KK_PI((pi_sweep<OffT, VT>(h, n, lpr, A_rm, A_ent, A_val, L.rm.as<OffT>(), L.ent.as<int32_t>(), L.val.as<VT>(), U.rm.as<OffT>(), U.ent.as<int32_t>(), U.val.as<VT>(),
                              Ut.rm.as<OffT>(), Ut.ent.as<int32_t>(), Ut.val.as<VT>(), st)));
    tick(3);
    // 7. the residual over A's pattern and the stop test
    if (do_residual) {
      KK_PI((pi_product<OffT, VT>(h, n, lpr, st)));
      tick(0);
      KK_PI((pi_residual<OffT, VT>(h, n, lpr, A_rm, A_ent, A_val, LU.rm.as<OffT>(), LU.ent.as<int32_t>(), LU.val.as<VT>(), d_scal + 2, st)));
      VT ss = VT(0);
      KK_HIP(hipMemcpyAsync(&ss, d_scal + 2, sizeof(VT), hipMemcpyDeviceToHost, st));
      KK_HIP(hipStreamSynchronize(st));
      ++h->host_syncs;
      curr = std::sqrt(ss);
      tick(6);
      if (h->verbose) std::cout << "Completed itr " << itr << ", residual is: " << curr << std::endl;
      if (std::abs(prev - curr) <= (VT)h->residual_norm_delta_stop) {
        if (h->verbose) std::cout << "  Itr-to-itr residual change has dropped below residual_norm_delta_stop, stop" << std::endl;
        stop = true;
      } else {
        prev = curr;
      }
    } else {
      curr = VT(0); prev = VT(0);
    }
    ++itr;
  }
  if (n == 0) curr = VT(0);
  if (h->verbose) {
    if (do_residual) std::cout << "PAR_ILUT stopped in " << itr << " iterations with residual " << curr << std::endl;
    else std::cout << "PAR_ILUT stopped in " << itr << " iterations with unknown residual" << std::endl;
  }
  KK_HIP(hipMemcpyAsync(L_rm_out, L.rm.p, rmb, hipMemcpyDeviceToDevice, st));
  KK_HIP(hipMemcpyAsync(U_rm_out, U.rm.p, rmb, hipMemcpyDeviceToDevice, st));
  KK_HIP(hipStreamSynchronize(st));
  ++h->host_syncs;
  h->num_iters = itr;
  h->end_rel_res = (double)curr;
  return KKAMD_OK;
}

template <class OffT>
static int pi_symbolic_typed(kkamd_par_ilut_handle* h, int64_t n, const OffT* A_rm, const int32_t* A_ent, OffT* L_rm, OffT* U_rm, hipStream_t st) {
  std::vector<OffT> rm((size_t)n + 1);
  KK_HIP(hipMemcpyAsync(rm.data(), A_rm, sizeof(OffT) * (size_t)(n + 1), hipMemcpyDeviceToHost, st));
  KK_HIP(hipStreamSynchronize(st));
  for (int64_t i = 0; i < n; ++i)
    if ((int64_t)rm[(size_t)i + 1] < (int64_t)rm[(size_t)i] || (int64_t)rm[(size_t)i] < 0)
      return fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_symbolic: row %lld: A's row_map offsets are not ascending", (long long)i);
  const int64_t a0 = (int64_t)rm[0], nnz = (int64_t)rm[(size_t)n] - a0;
  std::vector<int32_t> ent((size_t)nnz);
  if (nnz > 0) {
    if (!A_ent) return fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_symbolic: null entries");
    KK_HIP(hipMemcpyAsync(ent.data(), A_ent + a0, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, st));
    KK_HIP(hipStreamSynchronize(st));
  }
  for (int64_t i = 0; i < n; ++i) {
    const int64_t b = (int64_t)rm[(size_t)i] - a0, e = (int64_t)rm[(size_t)i + 1] - a0;
    for (int64_t p = b; p < e; ++p) {
      const int64_t c = ent[(size_t)p];
      if (c < 0 || c >= n)
        return fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_symbolic: row %lld: a column of A is outside [0, num_rows)", (long long)i);
      if (p > b && c <= (int64_t)ent[(size_t)p - 1])   // the reference asserts it inside add_candidates (numeric_impl.hpp:306)
        return fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_symbolic: row %lld: columns are not strictly ascending: add_candidates: Overflowed L_new, is your A matrix sorted?",
                    (long long)i);
    }
  }
  if (sizeof(OffT) == 4 && nnz + n > (int64_t)INT32_MAX)     // nnzL and nnzU are at most nnz(A) + n each
    return fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_symbolic: L or U may have more than 2^31 - 1 entries (nnz(A) %lld + %lld rows): use 64-bit offsets",
                (long long)nnz, (long long)n);
  h->nnzA = nnz;
  const int lpr = pi_lanes(h, n, nnz);
  KK_LAUNCH((pi_symbolic_kernel<OffT>), pi_grid(n + 1, lpr), kBlock, 0, st, n, lpr, pi_log2(lpr), A_rm, A_ent, L_rm, U_rm);
  KK_PI(pi_scan<OffT>(h, L_rm, n + 1, st));
  KK_PI(pi_scan<OffT>(h, U_rm, n + 1, st));
  KK_LAUNCH_CHECK();
  KK_PI(pi_read_totals<OffT>(h, L_rm, U_rm, n, &h->nnzL, &h->nnzU, st));
  KK_PI(pi_ensure(h, &h->sym_L_rm, sizeof(OffT) * (size_t)(n + 1)));
  KK_PI(pi_ensure(h, &h->sym_U_rm, sizeof(OffT) * (size_t)(n + 1)));
  KK_HIP(hipMemcpyAsync(h->sym_L_rm.p, L_rm, sizeof(OffT) * (size_t)(n + 1), hipMemcpyDeviceToDevice, st));
  KK_HIP(hipMemcpyAsync(h->sym_U_rm.p, U_rm, sizeof(OffT) * (size_t)(n + 1), hipMemcpyDeviceToDevice, st));
  KK_HIP(hipStreamSynchronize(st));
  return KKAMD_OK;
}

static int pi_check_types(const char* who, int offset_type, int value_type) {
  if (offset_type != KKAMD_I32 && offset_type != KKAMD_I64) return fail(KKAMD_ERR_INVALID_ARG, "%s: unknown offset_type %d", who, offset_type);
  if (value_type != KKAMD_F64 && value_type != KKAMD_F32) return fail(KKAMD_ERR_UNSUPPORTED, "%s: unsupported value_type %d: F64 and F32 are", who, value_type);
  return KKAMD_OK;
}

}  // namespace kk

// OT, VT over the four type pairs
#define KK_PI_DISPATCH(offset_type, value_type, CALL)                         \
  do {                                                                        \
    if ((offset_type) == KKAMD_I64) {                                         \
      if ((value_type) == KKAMD_F64) { typedef int64_t OT; typedef double VT; return CALL; } \
      { typedef int64_t OT; typedef float VT; return CALL; }                  \
    }                                                                         \
    if ((value_type) == KKAMD_F64) { typedef int32_t OT; typedef double VT; return CALL; }   \
    { typedef int32_t OT; typedef float VT; return CALL; }                    \
  } while (0)

extern "C" {

int kkamd_par_ilut_create(kkamd_par_ilut_handle_t** handle, int64_t max_iter, double residual_norm_delta_stop, double fill_in_limit, int async_update,
                          int verbose) {
  if (!handle) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_create: null handle pointer");
  *handle = nullptr;
  if (max_iter < 0) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_create: max_iter %lld is negative", (long long)max_iter);
  if (!(fill_in_limit >= 0)) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_create: fill_in_limit %g is negative", fill_in_limit);
  if (residual_norm_delta_stop != residual_norm_delta_stop) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_create: residual_norm_delta_stop is NaN");
  kkamd_par_ilut_handle* h = new (std::nothrow) kkamd_par_ilut_handle();
  if (!h) return kk::fail(KKAMD_ERR_ALLOC, "kkamd_par_ilut_create: out of host memory");
  const int rc = kkamd_spgemm_create(&h->spgemm);
  if (rc) { delete h; return rc; }
  h->max_iter = max_iter;
  h->residual_norm_delta_stop = residual_norm_delta_stop;
  h->fill_in_limit = fill_in_limit;
  h->async_update = async_update ? 1 : 0;
  h->verbose = verbose ? 1 : 0;
  *handle = h;
  return KKAMD_OK;
}

int kkamd_par_ilut_destroy(kkamd_par_ilut_handle_t* h) {
  if (!h) return KKAMD_OK;
  if (h->spgemm) (void)kkamd_spgemm_destroy(h->spgemm);
  for (kk::PiCsr* m : {&h->L, &h->U, &h->Ln, &h->Un, &h->Ut, &h->LU})
    for (kk::PiBuf* b : {&m->rm, &m->ent, &m->val}) kk::pi_free(h, b);
  for (kk::PiBuf* b : {&h->pre, &h->scanws, &h->rowsum, &h->sel, &h->scal, &h->sym_L_rm, &h->sym_U_rm}) kk::pi_free(h, b);
  delete h;
  return KKAMD_OK;
}

int kkamd_par_ilut_symbolic(kkamd_par_ilut_handle_t* h, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries, void* d_L_row_map,
                            void* d_U_row_map, int offset_type, kkamd_stream_t stream) {
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_symbolic: null handle");
  if (num_rows < 0 || num_rows >= (int64_t)INT32_MAX)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_symbolic: num_rows %lld is outside [0, 2^31 - 1)", (long long)num_rows);
  if (offset_type != KKAMD_I32 && offset_type != KKAMD_I64) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_symbolic: unknown offset_type %d", offset_type);
  if (!d_A_row_map || !d_L_row_map || !d_U_row_map) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_symbolic: null row_map");
  kk::TraceRange range("KokkosSparse::par_ilut_symbolic[TPL_KKAMD]");
  hipStream_t st = kk::to_hip(stream);
  h->symbolic_complete = false; h->numeric_complete = false;
  const int rc = offset_type == KKAMD_I64
                     ? kk::pi_symbolic_typed<int64_t>(h, num_rows, (const int64_t*)d_A_row_map, d_A_entries, (int64_t*)d_L_row_map, (int64_t*)d_U_row_map, st)
                     : kk::pi_symbolic_typed<int32_t>(h, num_rows, (const int32_t*)d_A_row_map, d_A_entries, (int32_t*)d_L_row_map, (int32_t*)d_U_row_map, st);
  if (rc) return rc;
  h->nrows = num_rows;
  h->offset_type = offset_type;
  h->symbolic_complete = true;
  return KKAMD_OK;
}

int kkamd_par_ilut_numeric(kkamd_par_ilut_handle_t* h, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries, const void* d_A_values,
                           void* d_L_row_map, void* d_U_row_map, int offset_type, int value_type, kkamd_stream_t stream) {
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_numeric: null handle");
  if (!h->symbolic_complete)
    return kk::fail(KKAMD_ERR_STATE, "KokkosSparse::Experimental::par_ilut_numeric: the symbolic phase has not been completed on this handle");
  const int rt = kk::pi_check_types("kkamd_par_ilut_numeric", offset_type, value_type);
  if (rt) return rt;
  if (num_rows != h->nrows)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_numeric: num_rows %lld differs from the symbolic call's %lld", (long long)num_rows, (long long)h->nrows);
  if (offset_type != h->offset_type) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_numeric: offset_type differs from the symbolic call's");
  if (!d_A_row_map || !d_L_row_map || !d_U_row_map || (h->nnzA > 0 && (!d_A_entries || !d_A_values)))
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_numeric: null pointer");
  kk::TraceRange range(value_type == KKAMD_F64 ? "KokkosSparse::par_ilut_numeric[TPL_KKAMD,double]" : "KokkosSparse::par_ilut_numeric[TPL_KKAMD,float]");
  hipStream_t st = kk::to_hip(stream);
  h->numeric_complete = false;
  int rc;
  if (offset_type == KKAMD_I64)
    rc = value_type == KKAMD_F64 ? kk::pi_numeric_typed<int64_t, double>(h, num_rows, (const int64_t*)d_A_row_map, d_A_entries, (const double*)d_A_values,
                                                                         (int64_t*)d_L_row_map, (int64_t*)d_U_row_map, st)
                                 : kk::pi_numeric_typed<int64_t, float>(h, num_rows, (const int64_t*)d_A_row_map, d_A_entries, (const float*)d_A_values,
                                                                        (int64_t*)d_L_row_map, (int64_t*)d_U_row_map, st);
  else
    rc = value_type == KKAMD_F64 ? kk::pi_numeric_typed<int32_t, double>(h, num_rows, (const int32_t*)d_A_row_map, d_A_entries, (const double*)d_A_values,
                                                                         (int32_t*)d_L_row_map, (int32_t*)d_U_row_map, st)
                                 : kk::pi_numeric_typed<int32_t, float>(h, num_rows, (const int32_t*)d_A_row_map, d_A_entries, (const float*)d_A_values,
                                                                        (int32_t*)d_L_row_map, (int32_t*)d_U_row_map, st);
  if (rc) return rc;
  h->value_type = value_type;
  h->numeric_complete = true;
  return KKAMD_OK;
}

int kkamd_par_ilut_copy_factors(kkamd_par_ilut_handle_t* h, int32_t* d_L_entries, void* d_L_values, int64_t L_capacity, int32_t* d_U_entries, void* d_U_values,
                                int64_t U_capacity, kkamd_stream_t stream) {
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_copy_factors: null handle");
  if (!h->numeric_complete)
    return kk::fail(KKAMD_ERR_STATE, "kkamd_par_ilut_copy_factors: the numeric phase has not been completed on this handle");
  if (L_capacity < h->L.nnz)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_copy_factors: L_entries's extent %lld is too small, must be at least %lld", (long long)L_capacity,
                    (long long)h->L.nnz);
  if (U_capacity < h->U.nnz)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_copy_factors: U_entries's extent %lld is too small, must be at least %lld", (long long)U_capacity,
                    (long long)h->U.nnz);
  if ((h->L.nnz > 0 && (!d_L_entries || !d_L_values)) || (h->U.nnz > 0 && (!d_U_entries || !d_U_values)))
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_copy_factors: null pointer");
  hipStream_t st = kk::to_hip(stream);
  const size_t vsz = h->value_type == KKAMD_F64 ? 8 : 4;
  if (h->L.nnz > 0) {
    KK_HIP(hipMemcpyAsync(d_L_entries, h->L.ent.p, sizeof(int32_t) * (size_t)h->L.nnz, hipMemcpyDeviceToDevice, st));
    KK_HIP(hipMemcpyAsync(d_L_values, h->L.val.p, vsz * (size_t)h->L.nnz, hipMemcpyDeviceToDevice, st));
  }
  if (h->U.nnz > 0) {
    KK_HIP(hipMemcpyAsync(d_U_entries, h->U.ent.p, sizeof(int32_t) * (size_t)h->U.nnz, hipMemcpyDeviceToDevice, st));
    KK_HIP(hipMemcpyAsync(d_U_values, h->U.val.p, vsz * (size_t)h->U.nnz, hipMemcpyDeviceToDevice, st));
  }
  return KKAMD_OK;
}

int kkamd_par_ilut_set(kkamd_par_ilut_handle_t* h, const char* key, double value) {
  if (!h || !key) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_set: null argument");
  const std::string k(key);
  const bool whole = value == std::floor(value);
  if (k == "max_iter") {
    if (!whole || value < 0) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_set: max_iter must be a whole number >= 0");
    h->max_iter = (int64_t)value;
  } else if (k == "residual_norm_delta_stop") {
    if (value != value) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_set: residual_norm_delta_stop is NaN");
    h->residual_norm_delta_stop = value;
  } else if (k == "fill_in_limit") {
    if (!(value >= 0)) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_set: fill_in_limit must be >= 0");
    h->fill_in_limit = value;
  } else if (k == "async_update") {
    if (value != 0 && value != 1) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_set: async_update is 0 or 1");
    h->async_update = (int)value;
  } else if (k == "verbose") {
    if (value != 0 && value != 1) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_set: verbose is 0 or 1");
    h->verbose = (int)value;
  } else if (k == "profile") {
    if (value != 0 && value != 1) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_set: profile is 0 or 1");
    h->profile = (int)value;
  } else if (k == "lanes_per_row") {
    const int v = (int)value;
    if (!whole || value < 0 || value > 64 || (v & (v - 1))) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_set: lanes_per_row is 0 or a power of two up to 64");
    h->lanes_per_row = v;
  } else {
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_set: unknown key '%s'", key);
  }
  return KKAMD_OK;
}

int kkamd_par_ilut_get(const kkamd_par_ilut_handle_t* h, const char* key, int64_t* value) {
  if (!h || !key || !value) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_get: null argument");
  const std::string k(key);
  if (k == "num_iters") *value = h->num_iters;
  else if (k == "nnzL") *value = h->nnzL;
  else if (k == "nnzU") *value = h->nnzU;
  else if (k == "nnzL_out") *value = h->numeric_complete ? h->L.nnz : 0;
  else if (k == "nnzU_out") *value = h->numeric_complete ? h->U.nnz : 0;
  else if (k == "num_rows") *value = h->nrows;
  else if (k == "symbolic_complete") *value = h->symbolic_complete ? 1 : 0;
  else if (k == "numeric_complete") *value = h->numeric_complete ? 1 : 0;
  else if (k == "max_iter") *value = h->max_iter;
  else if (k == "async_update") *value = h->async_update;
  else if (k == "verbose") *value = h->verbose;
  else if (k == "lanes_per_row") *value = h->lanes_per_row;
  else if (k == "profile") *value = h->profile;
  else if (k == "lanes_in_use") *value = kk::pi_lanes(h, h->nrows, h->nnzA);
  else if (k == "stage_entries_per_lane") *value = kk::kPiStage;
  else if (k == "plan_bytes") *value = h->bytes;
  else if (k == "host_syncs") *value = h->host_syncs;
  else if (k == "launches") *value = h->launches;
  else if (k == "max_product_row") *value = h->max_product_row;
  else return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_get: unknown key '%s'", key);
  return KKAMD_OK;
}

int kkamd_par_ilut_get_real(const kkamd_par_ilut_handle_t* h, const char* key, double* value) {
  if (!h || !key || !value) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_get_real: null argument");
  const std::string k(key);
  if (k == "end_rel_res") *value = h->end_rel_res;
  else if (k == "l_threshold") *value = h->l_threshold;
  else if (k == "u_threshold") *value = h->u_threshold;
  else if (k == "residual_norm_delta_stop") *value = h->residual_norm_delta_stop;
  else if (k == "fill_in_limit") *value = h->fill_in_limit;
  else if (k == "product_ms") *value = h->step_ms[0];
  else if (k == "candidates_ms") *value = h->step_ms[1];
  else if (k == "transpose_ms") *value = h->step_ms[2];
  else if (k == "sweep_ms") *value = h->step_ms[3];
  else if (k == "select_ms") *value = h->step_ms[4];
  else if (k == "filter_ms") *value = h->step_ms[5];
  else if (k == "residual_ms") *value = h->step_ms[6];
  else return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_get_real: unknown key '%s'", key);
  return KKAMD_OK;
}

// ---- the steps on caller-held arrays
int kkamd_par_ilut_add_candidates(kkamd_par_ilut_handle_t* h, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries, const void* d_A_values,
                                  const void* d_L_row_map, const int32_t* d_L_entries, const void* d_L_values, const void* d_U_row_map,
                                  const int32_t* d_U_entries, const void* d_U_values, const void* d_LU_row_map, const int32_t* d_LU_entries,
                                  const void* d_LU_values, int64_t nnzLU, void* d_Ln_row_map, int32_t* d_Ln_entries, void* d_Ln_values, int64_t Ln_capacity,
                                  void* d_Un_row_map, int32_t* d_Un_entries, void* d_Un_values, int64_t Un_capacity, int64_t* nnzLn, int64_t* nnzUn,
                                  int offset_type, int value_type, kkamd_stream_t stream) {
  if (!h || !nnzLn || !nnzUn) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_add_candidates: null argument");
  const int rt = kk::pi_check_types("kkamd_par_ilut_add_candidates", offset_type, value_type);
  if (rt) return rt;
  if (num_rows < 0 || nnzLU < 0) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_add_candidates: negative size");
  if (!d_A_row_map || !d_L_row_map || !d_U_row_map || !d_LU_row_map || !d_Ln_row_map || !d_Un_row_map)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_add_candidates: null row_map");
  hipStream_t st = kk::to_hip(stream);
  const int lpr = h->lanes_per_row ? h->lanes_per_row : 8;
#define KK_PI_BODY(OT, VT)                                                                                                                              \
  do {                                                                                                                                                  \
    int rc = kk::pi_candidates_count<OT, VT>(h, num_rows, lpr, (const OT*)d_A_row_map, d_A_entries, (const OT*)d_LU_row_map, d_LU_entries, nnzLU, -1, \
                                             (OT*)d_Ln_row_map, (OT*)d_Un_row_map, nnzLn, nnzUn, st);                                                  \
    if (rc) return rc;                                                                                                                                  \
    if (!d_Ln_entries && !d_Un_entries) return KKAMD_OK;                                                                                               \
    if (*nnzLn > Ln_capacity || *nnzUn > Un_capacity)                                                                                                  \
      return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_add_candidates: capacities %lld / %lld are too small, must be at least %lld / %lld",      \
                      (long long)Ln_capacity, (long long)Un_capacity, (long long)*nnzLn, (long long)*nnzUn);                                           \
    if (!d_Ln_entries || !d_Ln_values || !d_Un_entries || !d_Un_values) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_add_candidates: null output"); \
    rc = kk::pi_candidates_fill<OT, VT>(h, num_rows, lpr, (const OT*)d_A_row_map, d_A_entries, (const VT*)d_A_values, (const OT*)d_L_row_map, d_L_entries, \
                                        (const VT*)d_L_values, (const OT*)d_U_row_map, d_U_entries, (const VT*)d_U_values, (const OT*)d_LU_row_map,    \
                                        d_LU_entries, (const VT*)d_LU_values, (const OT*)d_Ln_row_map, d_Ln_entries, (VT*)d_Ln_values,                 \
                                        (const OT*)d_Un_row_map, d_Un_entries, (VT*)d_Un_values, st);                                                  \
    if (rc) return rc;                                                                                                                                  \
    KK_HIP(hipStreamSynchronize(st));                                                                                                                   \
    return KKAMD_OK;                                                                                                                                    \
  } while (0)
  if (offset_type == KKAMD_I64) { if (value_type == KKAMD_F64) KK_PI_BODY(int64_t, double); KK_PI_BODY(int64_t, float); }
  if (value_type == KKAMD_F64) KK_PI_BODY(int32_t, double);
  KK_PI_BODY(int32_t, float);
#undef KK_PI_BODY
}

int kkamd_par_ilut_sweep(kkamd_par_ilut_handle_t* h, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries, const void* d_A_values,
                         const void* d_L_row_map, const int32_t* d_L_entries, void* d_L_values, const void* d_U_row_map, const int32_t* d_U_entries,
                         void* d_U_values, const void* d_Ut_row_map, const int32_t* d_Ut_entries, const void* d_Ut_values, int offset_type, int value_type,
                         kkamd_stream_t stream) {
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_sweep: null handle");
  const int rt = kk::pi_check_types("kkamd_par_ilut_sweep", offset_type, value_type);
  if (rt) return rt;
  if (num_rows < 0) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_sweep: negative size");
  if (num_rows == 0) return KKAMD_OK;
  if (!d_A_row_map || !d_L_row_map || !d_U_row_map || !d_Ut_row_map || !d_L_entries || !d_L_values || !d_U_entries || !d_U_values || !d_Ut_entries || !d_Ut_values)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_sweep: null pointer");
  hipStream_t st = kk::to_hip(stream);
  const int lpr = h->lanes_per_row ? h->lanes_per_row : 8;
  KK_PI_DISPATCH(offset_type, value_type,
                 (kk::pi_sweep<OT, VT>(h, num_rows, lpr, (const OT*)d_A_row_map, d_A_entries, (const VT*)d_A_values, (const OT*)d_L_row_map, d_L_entries,
                                       (VT*)d_L_values, (const OT*)d_U_row_map, d_U_entries, (VT*)d_U_values, (const OT*)d_Ut_row_map, d_Ut_entries,
                                       (const VT*)d_Ut_values, st)));
}

int kkamd_par_ilut_select(kkamd_par_ilut_handle_t* h, int64_t count, const void* d_values, int64_t rank, void* d_threshold, int value_type,
                          kkamd_stream_t stream) {
  if (!h) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_select: null handle");
  const int rt = kk::pi_check_types("kkamd_par_ilut_select", KKAMD_I32, value_type);
  if (rt) return rt;
  if (count <= 0 || rank < 0 || rank >= count)
    return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_select: rank %lld is outside [0, %lld)", (long long)rank, (long long)count);
  if (!d_values || !d_threshold) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_select: null pointer");
  hipStream_t st = kk::to_hip(stream);
  if (value_type == KKAMD_F64) return kk::pi_select<double>(h, (const double*)d_values, count, rank, (double*)d_threshold, st);
  return kk::pi_select<float>(h, (const float*)d_values, count, rank, (float*)d_threshold, st);
}

int kkamd_par_ilut_filter(kkamd_par_ilut_handle_t* h, int64_t num_rows, const void* d_I_row_map, const int32_t* d_I_entries, const void* d_I_values,
                          const void* d_threshold, void* d_O_row_map, int32_t* d_O_entries, void* d_O_values, int64_t O_capacity, int64_t* nnz_out,
                          int offset_type, int value_type, kkamd_stream_t stream) {
  if (!h || !nnz_out) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_filter: null argument");
  const int rt = kk::pi_check_types("kkamd_par_ilut_filter", offset_type, value_type);
  if (rt) return rt;
  if (num_rows < 0) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_filter: negative size");
  if (!d_I_row_map || !d_O_row_map || !d_threshold) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_filter: null pointer");
  hipStream_t st = kk::to_hip(stream);
  const int lpr = h->lanes_per_row ? h->lanes_per_row : 8;
#define KK_PI_BODY(OT, VT)                                                                                                                             \
  do {                                                                                                                                                 \
    int rc = kk::pi_filter_count<OT, VT>(h, num_rows, lpr, (const OT*)d_I_row_map, d_I_entries, (const VT*)d_I_values, (const VT*)d_threshold,        \
                                         (OT*)d_O_row_map, st);                                                                                       \
    if (rc) return rc;                                                                                                                                 \
    rc = kk::pi_read_totals<OT>(h, (const OT*)d_O_row_map, (const OT*)nullptr, num_rows, nnz_out, nullptr, st);                                       \
    if (rc) return rc;                                                                                                                                 \
    if (!d_O_entries) return KKAMD_OK;                                                                                                                 \
    if (*nnz_out > O_capacity)                                                                                                                        \
      return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_filter: capacity %lld is too small, must be at least %lld", (long long)O_capacity,       \
                      (long long)*nnz_out);                                                                                                           \
    if (!d_O_values) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_filter: null output");                                                    \
    rc = kk::pi_filter_fill<OT, VT>(h, num_rows, lpr, (const OT*)d_I_row_map, d_I_entries, (const VT*)d_I_values, (const VT*)d_threshold,             \
                                    (const OT*)d_O_row_map, d_O_entries, (VT*)d_O_values, st);                                                        \
    if (rc) return rc;                                                                                                                                 \
    KK_HIP(hipStreamSynchronize(st));                                                                                                                  \
    return KKAMD_OK;                                                                                                                                   \
  } while (0)
  if (offset_type == KKAMD_I64) { if (value_type == KKAMD_F64) KK_PI_BODY(int64_t, double); KK_PI_BODY(int64_t, float); }
  if (value_type == KKAMD_F64) KK_PI_BODY(int32_t, double);
  KK_PI_BODY(int32_t, float);
#undef KK_PI_BODY
}

int kkamd_par_ilut_residual(kkamd_par_ilut_handle_t* h, int64_t num_rows, const void* d_A_row_map, const int32_t* d_A_entries, const void* d_A_values,
                            const void* d_LU_row_map, const int32_t* d_LU_entries, const void* d_LU_values, double* residual_norm, int offset_type,
                            int value_type, kkamd_stream_t stream) {
  if (!h || !residual_norm) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_residual: null argument");
  const int rt = kk::pi_check_types("kkamd_par_ilut_residual", offset_type, value_type);
  if (rt) return rt;
  if (num_rows < 0) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_residual: negative size");
  *residual_norm = 0;
  if (num_rows == 0) return KKAMD_OK;
  if (!d_A_row_map || !d_LU_row_map) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_par_ilut_residual: null row_map");
  hipStream_t st = kk::to_hip(stream);
  const int lpr = h->lanes_per_row ? h->lanes_per_row : 8;
  const int rc0 = kk::pi_ensure(h, &h->scal, 4 * sizeof(double));
  if (rc0) return rc0;
#define KK_PI_BODY(OT, VT)                                                                                                                              \
  do {                                                                                                                                                  \
    const int rc = kk::pi_residual<OT, VT>(h, num_rows, lpr, (const OT*)d_A_row_map, d_A_entries, (const VT*)d_A_values, (const OT*)d_LU_row_map,      \
                                           d_LU_entries, (const VT*)d_LU_values, h->scal.as<VT>() + 2, st);                                            \
    if (rc) return rc;                                                                                                                                  \
    VT ss = VT(0);                                                                                                                                      \
    KK_HIP(hipMemcpyAsync(&ss, h->scal.as<VT>() + 2, sizeof(VT), hipMemcpyDeviceToHost, st));                                                          \
    KK_HIP(hipStreamSynchronize(st));                                                                                                                   \
    *residual_norm = (double)std::sqrt(ss);                                                                                                             \
    return KKAMD_OK;                                                                                                                                    \
  } while (0)
  if (offset_type == KKAMD_I64) { if (value_type == KKAMD_F64) KK_PI_BODY(int64_t, double); KK_PI_BODY(int64_t, float); }
  if (value_type == KKAMD_F64) KK_PI_BODY(int32_t, double);
  KK_PI_BODY(int32_t, float);
#undef KK_PI_BODY
}

}  // extern "C"
