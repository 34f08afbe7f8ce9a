// kk_mis2.hip -- distance-2 maximal independent set, MIS-2 aggregation and explicit graph coarsening: KokkosGraph::graph_d2_mis /
// graph_mis2_coarsen / graph_mis2_aggregate (graph/src/KokkosGraph_MIS2.hpp; native implementation
// graph/impl/KokkosGraph_Distance2MIS_impl.hpp: MIS2_FAST :30-470, MIS2_QUALITY :472-793, the aggregation :795-1114) and
// KokkosGraph::Experimental::graph_explicit_coarsen (graph/src/KokkosGraph_ExplicitCoarsening.hpp) for a symmetric CRS graph.
//
// One round of the MIS-2 is four launches and one host synchronisation (the reference: five launches and two blocking scans).
//   1. mis2_col_kernel: a group of L lanes per entry of the column work list takes the minimum row status over the column and its
//      neighbours (IN_SET becomes OUT_SET) and stores it; the columns that stay live (status != OUT_SET) are ranked inside the
//      workgroup by ballot / popcount and written, in work-list order, to the workgroup's piece of `tmp`; the workgroup's count goes
//      to `counts`.
//   2. mis2_row_kernel: the same for the row work list: a row becomes OUT_SET when a column of its closed neighbourhood is OUT_SET,
//      IN_SET when all of them carry its own status; the rows still undecided are ranked and written the same way.
//   3. one exclusive scan (kk_scan.h) over the counts of both kernels' workgroups, the columns' first.
//   4. mis2_move_kernel: every piece goes to its offset in the work list it came from -- both lists stay in ascending vertex order, no
//      cursor, no returning atomic -- and, under MIS2_FAST, the surviving rows get the status of the next round, so no launch is spent
//      on the refresh.  Its first work-item leaves the two lengths where the host reads them.
// The host reads the lengths (one synchronisation), stops at an empty row list, and fails when a round decided no row: on a symmetric
// graph the undecided row of smallest status is decided in every round, so a round without progress proves the graph unsymmetric
// (the reference loops forever there).  MIS2_QUALITY runs the same round with fixed row statuses: refreshing every live column gives
// the statuses of the reference's refresh-by-bitset, because a column's minimum changes only when the row that holds it is decided.
// The set is compacted in ascending vertex order by the same ranking; its size is counted by the row kernel (integer atomics).
// The lanes per work-list entry L only split a row's entries among lanes; minima, ORs and integer sums do not depend on the split.
// No work-item waits on another workgroup; no floating-point atomic; the temporaries of a call are one kk::DevBuf.
#include "kk_scan.h"
#include <climits>
#include <cstring>

namespace kk {

constexpr uint32_t kMisIn = 0u, kMisOut = 0xFFFFFFFFu;
constexpr unsigned long long kMisNoError = ~0ull;
enum { kCtrBad = 0, kCtrMinDeg = 1, kCtrMaxDeg = 2, kCtrInSet = 3, kCtrUnlabelled = 4, kCtrTotal = 5, kCtrColLen = 6, kCtrRowLen = 7, kCtrCount = 8 };
constexpr int kMisLanes = 8;                                // lanes per row of the validation

// xorshiftHash<uint32_t> (common/src/KokkosKernels_SimpleUtils.hpp:377-385), stated bit for bit in kkamd.h
__host__ __device__ __forceinline__ uint32_t mis2_hash(uint32_t v) {
  uint64_t x = v;
  x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
  return (uint32_t)((x * 2685821657736338717ull - 1ull) >> 16);
}
// RefreshRowStatus (Distance2MIS_impl.hpp:80-90)
__device__ __forceinline__ uint32_t mis2_fast_status(int32_t i, uint32_t hashed_round, int nv_bits) {
  const uint32_t priority = mis2_hash(mis2_hash((uint32_t)i) ^ hashed_round);
  uint32_t s = (uint32_t)(i + 1) | (nv_bits < 32 ? priority << nv_bits : 0u);
  if (s == kMisOut) --s;
  return s;
}
// InitRowStatus (:533-546); equal degrees: the score is 0 (the reference divides by zero there)
__device__ __forceinline__ uint32_t mis2_quality_status(int32_t i, int32_t deg, int32_t min_deg, int32_t max_deg, int nv_bits) {
  const int deg_bits = 32 - nv_bits;
  if (deg_bits <= 0) return (uint32_t)(i + 1);
  const uint32_t max_deg_range = (1u << deg_bits) - 2u;
  float score = 0.f;
  if (max_deg > min_deg) {
    const float inv = 1.f / (float)(max_deg - min_deg);
    score = (float)(deg - min_deg) * inv;
  }
  const float scaled = score * (float)max_deg_range;
  return (uint32_t)(i + 1) + (((uint32_t)scaled) << nv_bits);
}

// Ranks the flagged work-items of a workgroup in thread order.  Every work-item of the workgroup calls it.
__device__ __forceinline__ int mis2_block_rank(bool flag, int* total, int* s_wave) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag ? 1 : 0);
  const int below = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();
  if (lane == 0) s_wave[w] = __popcll(m);
  __syncthreads();
  int base = 0, tot = 0;
  for (int k = 0; k < kBlock / 64; ++k) { const int sv = s_wave[k]; if (k < w) base += sv; tot += sv; }
  *total = tot;
  return base + below;
}

// ctr[kCtrBad]: the smallest offending row; with want_deg ctr[kCtrMinDeg], ctr[kCtrMaxDeg]: the degree range (row lengths, as the
// reference takes them), reduced over the wave first: a million atomics on one address cost more than the rounds
template <class OffT>
__global__ __launch_bounds__(kBlock) void mis2_validate_kernel(int64_t n, const OffT* __restrict__ rm, const int32_t* __restrict__ ent, int want_deg,
                                                               unsigned long long* __restrict__ ctr) {
  const int64_t r = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / kMisLanes;
  const int lane  = threadIdx.x & (kMisLanes - 1);
  const bool valid = r < n;
  int bad = 0;
  int64_t len = 0;
  if (valid) {
    const int64_t s = (int64_t)rm[r], e = (int64_t)rm[r + 1], last = (int64_t)rm[n];
    len = e - s;
    if (s < 0 || len < 0 || len > (int64_t)INT32_MAX || e > last) { bad = 1; len = 0; }
    for (int64_t j = s + lane; j < s + len; j += kMisLanes)
      if (ent[j] < 0) bad = 1;
  }
  for (int o = kMisLanes >> 1; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
  if (valid && lane == 0 && bad) atomicMin(&ctr[kCtrBad], (unsigned long long)r);
  if (!want_deg) return;                                     // uniform over the launch
  int lo = valid && !bad ? (int)len : INT32_MAX, hi = valid && !bad ? (int)len : 0;
  for (int o = 32; o > 0; o >>= 1) {
    const int lo2 = __shfl_xor(lo, o, 64), hi2 = __shfl_xor(hi, o, 64);
    lo = lo2 < lo ? lo2 : lo; hi = hi2 > hi ? hi2 : hi;
  }
  if ((threadIdx.x & 63) == 0 && lo <= hi) {
    atomicMin(&ctr[kCtrMinDeg], (unsigned long long)lo);
    atomicMax(&ctr[kCtrMaxDeg], (unsigned long long)hi);
  }
}

// The lists and statuses before round 0.  mask NULL: every row is in the row list.  Otherwise (the masked form, :385-397) the rows
// with mask < 0 are ranked into tmp / counts, the others are OUT_SET.  Every column is in the column list.
template <class OffT>
__global__ __launch_bounds__(kBlock) void mis2_init_kernel(int64_t n, const OffT* __restrict__ rm, const int32_t* __restrict__ mask, int quality,
                                                           int32_t min_deg, int32_t max_deg, int nv_bits, uint32_t hashed_round,
                                                           uint32_t* __restrict__ row_status, int32_t* __restrict__ row_list,
                                                           int32_t* __restrict__ col_list, int32_t* __restrict__ tmp, int64_t* __restrict__ counts) {
  __shared__ int s_wave[kBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool valid = i < n;
  const bool in_list = valid && (!mask || mask[i] < 0);
  if (valid) {
    col_list[i] = (int32_t)i;
    uint32_t s = kMisOut;
    if (in_list) s = quality ? mis2_quality_status((int32_t)i, (int32_t)((int64_t)rm[i + 1] - (int64_t)rm[i]), min_deg, max_deg, nv_bits)
                             : mis2_fast_status((int32_t)i, hashed_round, nv_bits);
    row_status[i] = s;
    if (!mask) row_list[i] = (int32_t)i;
  }
  if (!mask) return;                                         // uniform over the launch
  int total;
  const int rank = mis2_block_rank(in_list, &total, s_wave);
  if (in_list) tmp[(int64_t)blockIdx.x * kBlock + rank] = (int32_t)i;
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// RefreshColStatus (:109-125) for the entries [0, len) of the column list, and the ranking of the columns that stay live
template <class OffT>
__global__ __launch_bounds__(kBlock) void mis2_col_kernel(int64_t len, int lanes, int shift, const int32_t* __restrict__ col_list, int64_t n,
                                                          const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                          const uint32_t* __restrict__ row_status, uint32_t* __restrict__ col_status,
                                                          int32_t* __restrict__ tmp, int64_t* __restrict__ counts) {
  __shared__ int s_wave[kBlock / 64];
  const int64_t g = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> shift;
  const int lane  = threadIdx.x & (lanes - 1);
  const bool valid = g < len;
  uint32_t s = kMisOut;
  int32_t c = 0;
  if (valid) {
    c = col_list[g];
    if (lane == 0) s = row_status[c];
    const int64_t e = (int64_t)rm[c + 1];
    for (int64_t p = (int64_t)rm[c] + lane; p < e; p += lanes) {
      const int32_t j = ent[p];
      if (j < n) { const uint32_t sj = row_status[j]; s = sj < s ? sj : s; }
    }
  }
  for (int o = lanes >> 1; o > 0; o >>= 1) { const uint32_t s2 = __shfl_xor(s, o, 64); s = s2 < s ? s2 : s; }
  if (s == kMisIn) s = kMisOut;
  const bool lead = valid && lane == 0;
  if (lead) col_status[c] = s;
  const bool keep = lead && s != kMisOut;
  int total;
  const int rank = mis2_block_rank(keep, &total, s_wave);
  if (keep) tmp[(int64_t)blockIdx.x * (kBlock >> shift) + rank] = c;
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// DecideSetFunctor (:178-209) for the entries [0, len) of the row list, and the ranking of the rows still undecided
template <class OffT>
__global__ __launch_bounds__(kBlock) void mis2_row_kernel(int64_t len, int lanes, int shift, const int32_t* __restrict__ row_list, int64_t n,
                                                          const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                          uint32_t* __restrict__ row_status, const uint32_t* __restrict__ col_status,
                                                          int32_t* __restrict__ tmp, int64_t* __restrict__ counts, unsigned long long* __restrict__ ctr) {
  __shared__ int s_wave[kBlock / 64];
  __shared__ int s_in[kBlock / 64];
  const int64_t g = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> shift;
  const int lane  = threadIdx.x & (lanes - 1);
  const bool valid = g < len;
  int flags = 0;                                             // 1: a column is OUT_SET, 2: a column has another status
  int32_t i = 0;
  uint32_t s = 0;
  if (valid) {
    i = row_list[g];
    s = row_status[i];
    if (lane == 0) { const uint32_t cs = col_status[i]; flags |= cs == kMisOut ? 1 : (cs != s ? 2 : 0); }
    const int64_t e = (int64_t)rm[i + 1];
    for (int64_t p = (int64_t)rm[i] + lane; p < e; p += lanes) {
      const int32_t j = ent[p];
      if (j < n) { const uint32_t cs = col_status[j]; flags |= cs == kMisOut ? 1 : (cs != s ? 2 : 0); }
    }
  }
  for (int o = lanes >> 1; o > 0; o >>= 1) flags |= __shfl_xor(flags, o, 64);
  const bool lead = valid && lane == 0;
  const bool out = lead && (flags & 1), in = lead && flags == 0;
  if (out) row_status[i] = kMisOut;
  if (in) row_status[i] = kMisIn;
  const unsigned long long in_mask = __ballot(in ? 1 : 0);
  if ((threadIdx.x & 63) == 0) s_in[threadIdx.x >> 6] = __popcll(in_mask);
  const bool keep = lead && !out && !in;
  int total;
  const int rank = mis2_block_rank(keep, &total, s_wave);   // its barriers publish s_in
  if (keep) tmp[(int64_t)blockIdx.x * (kBlock >> shift) + rank] = i;
  if (threadIdx.x == 0) {
    counts[blockIdx.x] = total;
    int joined = 0;                                          // one atomic per workgroup on the one counter
    for (int k = 0; k < kBlock / 64; ++k) joined += s_in[k];
    if (joined) atomicAdd(&ctr[kCtrInSet], (unsigned long long)joined);
  }
}

// Piece b of tmp (group slots per piece, offs[b + 1] - offs[b] of them filled) goes to offs[b] of its list: pieces [0, nbc) are the column
// list's, [nbc, nbc + nbr) the row list's.  refresh: the moved rows get the status of the round whose hash is hashed_round.
__global__ __launch_bounds__(kBlock) void mis2_move_kernel(int64_t nbc, int64_t nbr, int group_shift, const int64_t* __restrict__ offs,
                                                           const int32_t* __restrict__ tmp, int32_t* __restrict__ col_list,
                                                           int32_t* __restrict__ row_list, int refresh, uint32_t hashed_round, int nv_bits,
                                                           uint32_t* __restrict__ row_status, unsigned long long* __restrict__ ctr) {
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q == 0) { ctr[kCtrColLen] = (unsigned long long)offs[nbc]; ctr[kCtrRowLen] = (unsigned long long)(offs[nbc + nbr] - offs[nbc]); }
  const int64_t b = q >> group_shift, t = q & (((int64_t)1 << group_shift) - 1);
  if (b >= nbc + nbr) return;
  const int64_t o = offs[b];
  if (t >= offs[b + 1] - o) return;
  const int32_t v = tmp[q];
  if (b < nbc) { col_list[o + t] = v; return; }
  row_list[o - offs[nbc] + t] = v;
  if (refresh) row_status[v] = mis2_fast_status(v, hashed_round, nv_bits);
}

// the set in ascending vertex order: ranks the vertices whose status is IN_SET
__global__ __launch_bounds__(kBlock) void mis2_set_kernel(int64_t n, const uint32_t* __restrict__ row_status, int32_t* __restrict__ tmp,
                                                          int64_t* __restrict__ counts) {
  __shared__ int s_wave[kBlock / 64];
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool in = i < n && row_status[i] == kMisIn;
  int total;
  const int rank = mis2_block_rank(in, &total, s_wave);
  if (in) tmp[(int64_t)blockIdx.x * kBlock + rank] = (int32_t)i;
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// Phase1Functor (:825-835): aggregate g is root set[g] and all its neighbours.  The roots of a symmetric graph share no neighbour; the
// atomic maximum only makes the result of an unsymmetric graph a function of the graph.
template <class OffT>
__global__ __launch_bounds__(kBlock) void mis2_phase1_kernel(int64_t cnt, int lanes, int shift, const int32_t* __restrict__ set, int64_t n,
                                                             const OffT* __restrict__ rm, const int32_t* __restrict__ ent, int32_t* labels,
                                                             int8_t* __restrict__ roots) {
  const int64_t g = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> shift;
  const int lane  = threadIdx.x & (lanes - 1);
  if (g >= cnt) return;
  const int32_t root = set[g];
  if (lane == 0) { roots[root] = 1; atomicMax(&labels[root], (int32_t)g); }
  const int64_t e = (int64_t)rm[root + 1];
  for (int64_t p = (int64_t)rm[root] + lane; p < e; p += lanes) {
    const int32_t j = ent[p];
    if (j < n) atomicMax(&labels[j], (int32_t)g);
  }
}

// CandAggSizesFunctor (:864-876) and the ranking of the candidates with at least 3 unlabelled vertices in their closed neighbourhood
template <class OffT>
__global__ __launch_bounds__(kBlock) void mis2_cand_kernel(int64_t cnt, int lanes, int shift, const int32_t* __restrict__ cand, int64_t n,
                                                           const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                           const int32_t* __restrict__ labels, int32_t* __restrict__ tmp, int64_t* __restrict__ counts) {
  __shared__ int s_wave[kBlock / 64];
  const int64_t g = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> shift;
  const int lane  = threadIdx.x & (lanes - 1);
  const bool valid = g < cnt;
  int size = 0;
  int32_t root = 0;
  if (valid) {
    root = cand[g];
    if (lane == 0) size = 1;
    const int64_t e = (int64_t)rm[root + 1];
    for (int64_t p = (int64_t)rm[root] + lane; p < e; p += lanes) {
      const int32_t j = ent[p];
      if (j != root && j < n && labels[j] == -1) ++size;
    }
  }
  size = group_sum(size, lanes);
  const bool keep = valid && lane == 0 && size >= 3;
  int total;
  const int rank = mis2_block_rank(keep, &total, s_wave);
  if (keep) tmp[(int64_t)blockIdx.x * (kBlock >> shift) + rank] = root;
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// ChoosePhase2AggsFunctor (:899-917): the chosen candidate at offs[b] + t becomes aggregate base + offs[b] + t
template <class OffT>
__global__ __launch_bounds__(kBlock) void mis2_phase2_kernel(int64_t nb, int group_shift, const int64_t* __restrict__ offs, const int32_t* __restrict__ tmp,
                                                             int64_t base, int64_t n, const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                             int32_t* labels, int8_t* __restrict__ roots, unsigned long long* __restrict__ ctr) {
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q == 0) ctr[kCtrTotal] = (unsigned long long)offs[nb];
  const int64_t b = q >> group_shift, t = q & (((int64_t)1 << group_shift) - 1);
  if (b >= nb) return;
  const int64_t o = offs[b];
  if (t >= offs[b + 1] - o) return;
  const int32_t root = tmp[q], id = (int32_t)(base + o + t);
  labels[root] = id;
  roots[root]  = 1;
  const int64_t e = (int64_t)rm[root + 1];
  for (int64_t p = (int64_t)rm[root]; p < e; ++p) {
    const int32_t j = ent[p];
    if (j != root && j < n) (void)atomicCAS(&labels[j], -1, id);
  }
}

// SizeAndConnectivityFunctor (:958-975), the frozen copy of the labels, and the count of the vertices still unlabelled
template <class OffT>
__global__ __launch_bounds__(kBlock) void mis2_connect_kernel(int64_t n, int lanes, int shift, const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                              const int32_t* __restrict__ labels, int32_t* __restrict__ labels_old,
                                                              int32_t* __restrict__ connect, int32_t* __restrict__ agg_sizes,
                                                              unsigned long long* __restrict__ ctr) {
  __shared__ int s_free[kBlock / 64];
  const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> shift;
  const int lane  = threadIdx.x & (lanes - 1);
  const bool valid = i < n;
  int c = 0;
  int32_t agg = -1;
  if (valid) {
    agg = labels[i];
    if (agg != -1) {
      const int64_t e = (int64_t)rm[i + 1];
      for (int64_t p = (int64_t)rm[i] + lane; p < e; p += lanes) {
        const int32_t j = ent[p];
        if (j != i && j < n && labels[j] == agg) ++c;
      }
    }
  }
  c = group_sum(c, lanes);
  const bool lead = valid && lane == 0;
  const unsigned long long free_mask = __ballot(lead && agg == -1 ? 1 : 0);
  if ((threadIdx.x & 63) == 0) s_free[threadIdx.x >> 6] = __popcll(free_mask);
  __syncthreads();
  if (threadIdx.x == 0) {                                    // one atomic per workgroup on the one counter
    int unlabelled = 0;
    for (int k = 0; k < kBlock / 64; ++k) unlabelled += s_free[k];
    if (unlabelled) atomicAdd(&ctr[kCtrUnlabelled], (unsigned long long)unlabelled);
  }
  if (!lead) return;
  labels_old[i] = agg;
  connect[i]    = c;
  if (agg != -1) atomicAdd(&agg_sizes[agg], 1);
}

// AssignLeftoverFunctor (:998-1058): one work-item per vertex walks the entries in stored order, tracks up to 8 neighbouring aggregates,
// stops at the ninth, and moves by: adjacent to a root > connectivity > smaller size, the first best winning
template <class OffT>
__global__ __launch_bounds__(kBlock) void mis2_assign_kernel(int64_t n, const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                             const int32_t* __restrict__ labels_old, const int32_t* __restrict__ connect,
                                                             const int32_t* __restrict__ agg_sizes, const int8_t* __restrict__ roots,
                                                             int32_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t agg = labels_old[i];
  if (roots[i]) { labels[i] = agg; return; }
  int32_t t_agg[8], t_con[8];
  int t_root[8];
  int tracked = 0;
  const int64_t e = (int64_t)rm[i + 1];
  for (int64_t p = (int64_t)rm[i]; p < e; ++p) {
    const int32_t j = ent[p];
    if (j == i || j >= n) continue;
    const int32_t na = labels_old[j];
    if (na == -1 || na == agg) continue;
    int id = -1;
    for (int k = 0; k < tracked; ++k)
      if (t_agg[k] == na) { id = k; break; }
    if (id == -1) {
      if (tracked == 8) break;
      id = tracked++;
      t_agg[id] = na; t_con[id] = 0; t_root[id] = 0;
    }
    if (roots[j]) t_root[id] = 1;
    t_con[id] += 1;
  }
  int best_root = agg >= 0 ? 1 : 0;
  int32_t best_agg = agg, best_con = connect[i], best_size = agg >= 0 ? agg_sizes[agg] : 0;
  for (int k = 0; k < tracked; ++k) {
    const int32_t s = agg_sizes[t_agg[k]];
    if (t_root[k] > best_root || (t_root[k] == best_root && (t_con[k] > best_con || (t_con[k] == best_con && s < best_size)))) {
      best_root = t_root[k]; best_con = t_con[k]; best_size = s; best_agg = t_agg[k];
    }
  }
  labels[i] = best_agg;
}

// explicit coarsening ------------------------------------------------------------------------------------------------------------------

// ctr[kCtrBad]: the smallest vertex whose label is outside [0, nc); sizes[l]: vertices of cluster l
__global__ __launch_bounds__(kBlock) void coarsen_labels_kernel(int64_t n, const int32_t* __restrict__ labels, int64_t nc, int32_t* __restrict__ sizes,
                                                                unsigned long long* __restrict__ ctr) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t l = labels[i];
  if (l < 0 || l >= nc) atomicMin(&ctr[kCtrBad], (unsigned long long)i);
  else atomicAdd(&sizes[l], 1);
}

__global__ __launch_bounds__(kBlock) void coarsen_scatter_kernel(int64_t n, const int32_t* __restrict__ labels, int32_t* __restrict__ cursor,
                                                                 int32_t* __restrict__ verts) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  verts[atomicAdd(&cursor[labels[i]], 1)] = (int32_t)i;     // every cluster's piece is sorted ascending afterwards
}

// cnt[p]: the entries of vertex verts[p] that lead to another cluster
template <class OffT>
__global__ __launch_bounds__(kBlock) void coarsen_count_kernel(int64_t n, int lanes, int shift, const int32_t* __restrict__ verts,
                                                               const OffT* __restrict__ rm, const int32_t* __restrict__ ent,
                                                               const int32_t* __restrict__ labels, OffT* __restrict__ cnt) {
  const int64_t p = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> shift;
  const int lane  = threadIdx.x & (lanes - 1);
  const bool valid = p < n;
  int c = 0;
  if (valid) {
    const int32_t v = verts[p], l = labels[v];
    const int64_t e = (int64_t)rm[v + 1];
    for (int64_t k = (int64_t)rm[v] + lane; k < e; k += lanes) {
      const int32_t j = ent[k];
      if (j < n && labels[j] != l) ++c;
    }
  }
  c = group_sum(c, lanes);
  if (p == n && lane == 0) cnt[n] = 0;
  if (valid && lane == 0) cnt[p] = (OffT)c;
}

template <class OffT>
__global__ __launch_bounds__(kBlock) void coarsen_rowmap_kernel(int64_t nc, const int32_t* __restrict__ inv_off, const OffT* __restrict__ start,
                                                                OffT* __restrict__ coarse_rm) {
  const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (c <= nc) coarse_rm[c] = start[inv_off[c]];
}

// the vertices of a cluster in ascending order, their entries in stored order, every cross-cluster entry kept
template <class OffT>
__global__ __launch_bounds__(kBlock) void coarsen_fill_kernel(int64_t n, const int32_t* __restrict__ verts, const OffT* __restrict__ rm,
                                                              const int32_t* __restrict__ ent, const int32_t* __restrict__ labels,
                                                              const OffT* __restrict__ start, int32_t* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= n) return;
  const int32_t v = verts[p], l = labels[v];
  int64_t at = (int64_t)start[p];
  const int64_t e = (int64_t)rm[v + 1];
  for (int64_t k = (int64_t)rm[v]; k < e; ++k) {
    const int32_t j = ent[k];
    if (j < n) { const int32_t lj = labels[j]; if (lj != l) out[at++] = lj; }
  }
}

// host side ------------------------------------------------------------------------------------------------------------------------------

static int mis2_log2(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }
static int64_t mis2_scan_launches(int64_t n) { return n <= kScanTile ? 1 : 2 + mis2_scan_launches(ceil_div(n, kScanTile)); }

// lanes per work-list vertex: the knob, else about four entries of the mean closed neighbourhood per lane, as the Gauss-Seidel sweeps
// choose
static int mis2_lane_rule(int64_t nnz, int64_t n) {
  if (g_mis2_lanes) return g_mis2_lanes;
  int lanes = 1;
  const int64_t want = ceil_div(nnz + n, 4 * n);
  while (lanes < kWave && lanes < want) lanes *= 2;
  return lanes;
}

// The one validation pass and its read-back (one synchronisation): hc receives the counters, *nnz the last row offset.
template <class OffT>
static int mis2_validate(const char* who, int64_t n, const OffT* rm, const int32_t* ent, int want_deg, unsigned long long* ctr, hipStream_t st,
                         unsigned long long* hc, int64_t* nnz) {
  KK_HIP(hipMemsetAsync(ctr, 0, sizeof(unsigned long long) * kCtrCount, st));
  KK_HIP(hipMemsetAsync(ctr, 0xFF, sizeof(unsigned long long) * 2, st));            // kCtrBad, kCtrMinDeg
  KK_LAUNCH((mis2_validate_kernel<OffT>), (unsigned)ceil_div(n * kMisLanes, kBlock), kBlock, 0, st, n, rm, ent, want_deg, ctr);
  KK_LAUNCH_CHECK();
  OffT h_nnz = 0;
  KK_HIP(hipMemcpyAsync(hc, ctr, sizeof(unsigned long long) * kCtrCount, hipMemcpyDeviceToHost, st));
  KK_HIP(hipMemcpyAsync(&h_nnz, rm + n, sizeof(OffT), hipMemcpyDeviceToHost, st));
  KK_HIP(hipStreamSynchronize(st));
  if (hc[kCtrBad] != kMisNoError)
    return fail(KKAMD_ERR_INVALID_ARG, "%s: row %lld: its row_map offsets are not ascending, or one of its entries is negative", who, (long long)hc[kCtrBad]);
  *nnz = (int64_t)h_nnz;
  return KKAMD_OK;
}

// One allocation for the temporaries of a call (a hipMalloc / hipFree pair costs more than a round on a million vertices): the pieces are
// handed out in order, 256-byte aligned; take() returns nullptr past the end.
struct Mis2Slab {
  DevBuf buf;
  size_t used = 0, size = 0;
  static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  hipError_t alloc(size_t bytes) { used = 0; size = bytes; return buf.alloc(bytes); }
  template <class T> T* take(size_t count) {
    T* p = reinterpret_cast<T*>(buf.as<char>() + used);
    used += padded(sizeof(T) * count);
    return used <= size ? p : nullptr;
  }
};

template <class OffT> struct Mis2 {
  int64_t n = 0;
  const OffT* rm = nullptr;
  const int32_t* ent = nullptr;
  hipStream_t st = nullptr;
  int lanes = 1, shift = 0, group = kBlock, nv_bits = 0;
  int32_t min_deg = 0, max_deg = 0;
  int64_t nnz = 0, launches = 0, syncs = 0, bytes = 0;
  // every temporary of a call comes from the slab; ctr is a second, small allocation: it is needed before the sizes are known
  Mis2Slab slab;
  DevBuf ctr_b;
  uint32_t *row_status = nullptr, *col_status = nullptr;
  int32_t *row_list = nullptr, *col_list = nullptr, *tmp = nullptr;
  int64_t *counts = nullptr, *ws = nullptr;
  unsigned long long* ctr = nullptr;

  static size_t padded(size_t bytes) { return Mis2Slab::padded(bytes); }
  template <class T> T* take(size_t count) { return slab.take<T>(count); }
  int scan(int64_t items) {
    launches += mis2_scan_launches(items);
    return exclusive_scan_inplace<int64_t>(counts, items, st, ws);
  }
  int read_ctr(unsigned long long* h) {
    KK_HIP(hipMemcpyAsync(h, ctr, sizeof(unsigned long long) * kCtrCount, hipMemcpyDeviceToHost, st));
    KK_HIP(hipStreamSynchronize(st));
    ++syncs;
    return KKAMD_OK;
  }

  // validation (one synchronisation), the lane rule, the scratch of the rounds and extra_bytes more for the caller's take<>()
  int setup(const char* who, int64_t n_, const OffT* rm_, const int32_t* ent_, hipStream_t st_, int want_deg, size_t extra_bytes = 0) {
    n = n_; rm = rm_; ent = ent_; st = st_;
    KK_HIP(ctr_b.alloc(sizeof(unsigned long long) * kCtrCount));
    bytes += (int64_t)(sizeof(unsigned long long) * kCtrCount);
    ctr = ctr_b.as<unsigned long long>();
    unsigned long long hc[kCtrCount];
    const int rc = mis2_validate<OffT>(who, n, rm, ent, want_deg, ctr, st, hc, &nnz);
    ++launches;
    ++syncs;
    if (rc) return rc;
    if (want_deg) { min_deg = (int32_t)hc[kCtrMinDeg]; max_deg = (int32_t)hc[kCtrMaxDeg]; }
    { uint32_t v = (uint32_t)(n + 1); nv_bits = 0; while (v) { v >>= 1; ++nv_bits; } }
    lanes = mis2_lane_rule(nnz, n);
    shift = mis2_log2(lanes);
    group = kBlock >> shift;
    const int64_t pieces = 2 * ceil_div(n, group) + 2;
    const size_t tmp_items = (size_t)(pieces * group > ceil_div(n, kBlock) * kBlock ? pieces * group : ceil_div(n, kBlock) * kBlock);
    const size_t ws_items = (size_t)scan_workspace_items(pieces);
    const size_t slab_size = 4 * padded(sizeof(int32_t) * (size_t)n) + padded(sizeof(int32_t) * tmp_items) + padded(sizeof(int64_t) * (size_t)pieces) +
                padded(sizeof(int64_t) * ws_items) + extra_bytes;
    KK_HIP(slab.alloc(slab_size));
    bytes += (int64_t)slab_size;
    row_status = take<uint32_t>((size_t)n); col_status = take<uint32_t>((size_t)n);
    row_list = take<int32_t>((size_t)n); col_list = take<int32_t>((size_t)n);
    tmp = take<int32_t>(tmp_items); counts = take<int64_t>((size_t)pieces); ws = take<int64_t>(ws_items);
    return KKAMD_OK;
  }

  // the rounds.  mask NULL: D2_MIS_RandomPriority::compute() / D2_MIS_FixedPriority::compute(); else compute(mask).  The set goes to
  // d_set (n entries of room) in ascending order.
  int run(const char* who, int quality, const int32_t* mask, int32_t* d_set, int64_t* rounds_out, int64_t* in_set_out) {
    unsigned long long hc[kCtrCount];
    int rc;
    uint32_t *rs = row_status, *cs = col_status;
    int32_t *rl = row_list, *cl = col_list, *tp = tmp;
    int64_t* cnt = counts;
    const int64_t nb0 = ceil_div(n, kBlock);
    KK_HIP(hipMemsetAsync(ctr + kCtrInSet, 0, sizeof(unsigned long long), st));
    KK_LAUNCH((mis2_init_kernel<OffT>), (unsigned)nb0, kBlock, 0, st, n, rm, mask, quality, min_deg, max_deg, nv_bits, mis2_hash(0u), rs, rl, cl, tp, cnt);
    ++launches;
    int64_t row_len = n, col_len = n, rounds = 0, in_set = 0;
    if (mask) {
      KK_HIP(hipMemsetAsync(cnt + nb0, 0, sizeof(int64_t), st));
      if ((rc = scan(nb0 + 1))) return rc;
      KK_LAUNCH(mis2_move_kernel, (unsigned)nb0, kBlock, 0, st, (int64_t)0, nb0, 8, (const int64_t*)cnt, (const int32_t*)tp, cl, rl, 0, 0u, nv_bits, rs, ctr);
      KK_LAUNCH_CHECK();
      ++launches;
      if ((rc = read_ctr(hc))) return rc;
      row_len = (int64_t)hc[kCtrRowLen];
    }
    while (row_len > 0) {
      const int64_t nbc = ceil_div(col_len, group), nbr = ceil_div(row_len, group);
      if (nbc > 0)
        KK_LAUNCH((mis2_col_kernel<OffT>), (unsigned)nbc, kBlock, 0, st, col_len, lanes, shift, (const int32_t*)cl, n, rm, ent, (const uint32_t*)rs, cs, tp, cnt);
      KK_LAUNCH((mis2_row_kernel<OffT>), (unsigned)nbr, kBlock, 0, st, row_len, lanes, shift, (const int32_t*)rl, n, rm, ent, rs, (const uint32_t*)cs,
                tp + nbc * group, cnt + nbc, ctr);
      KK_HIP(hipMemsetAsync(cnt + nbc + nbr, 0, sizeof(int64_t), st));
      launches += nbc > 0 ? 2 : 1;
      if ((rc = scan(nbc + nbr + 1))) return rc;
      ++rounds;
      KK_LAUNCH(mis2_move_kernel, (unsigned)ceil_div((nbc + nbr) * group, kBlock), kBlock, 0, st, nbc, nbr, 8 - shift, (const int64_t*)cnt, (const int32_t*)tp,
                cl, rl, quality ? 0 : 1, mis2_hash((uint32_t)rounds), nv_bits, rs, ctr);
      KK_LAUNCH_CHECK();
      ++launches;
      if ((rc = read_ctr(hc))) return rc;
      const int64_t left = (int64_t)hc[kCtrRowLen];
      if (left >= row_len)
        return fail(KKAMD_ERR_INVALID_ARG, "%s: graph is not symmetric (round %lld decided none of %lld rows)", who, (long long)rounds, (long long)row_len);
      row_len = left;
      col_len = (int64_t)hc[kCtrColLen];
      in_set  = (int64_t)hc[kCtrInSet];
    }
    if (in_set > 0) {
      KK_LAUNCH(mis2_set_kernel, (unsigned)nb0, kBlock, 0, st, n, (const uint32_t*)rs, tp, cnt);
      KK_HIP(hipMemsetAsync(cnt + nb0, 0, sizeof(int64_t), st));
      ++launches;
      if ((rc = scan(nb0 + 1))) return rc;
      KK_LAUNCH(mis2_move_kernel, (unsigned)nb0, kBlock, 0, st, (int64_t)0, nb0, 8, (const int64_t*)cnt, (const int32_t*)tp, cl, d_set, 0, 0u, nv_bits, rs, ctr);
      KK_LAUNCH_CHECK();
      ++launches;
    }
    *rounds_out = rounds;
    *in_set_out = in_set;
    return KKAMD_OK;
  }
};

static void mis2_stats(int64_t* stats, int64_t r1, int64_t r2, int64_t syncs, int64_t launches, int64_t primary, int64_t secondary, int64_t unlabelled,
                       int64_t bytes) {
  if (!stats) return;
  stats[0] = r1; stats[1] = r2; stats[2] = syncs; stats[3] = launches; stats[4] = primary; stats[5] = secondary; stats[6] = unlabelled; stats[7] = bytes;
}

template <class OffT>
static int d2_mis_typed(int64_t n, const OffT* rm, const int32_t* ent, int algorithm, int32_t* d_mis, int64_t* num_in_set, int64_t* stats, hipStream_t st) {
  Mis2<OffT> m;
  int rc = m.setup("kkamd_graph_d2_mis", n, rm, ent, st, algorithm == KKAMD_MIS2_QUALITY);
  if (rc) return rc;
  int64_t rounds = 0, in_set = 0;
  if ((rc = m.run("kkamd_graph_d2_mis", algorithm == KKAMD_MIS2_QUALITY, nullptr, d_mis, &rounds, &in_set))) return rc;
  KK_HIP(hipStreamSynchronize(st));
  ++m.syncs;
  *num_in_set = in_set;
  mis2_stats(stats, rounds, 0, m.syncs, m.launches, 0, 0, 0, m.bytes);
  return KKAMD_OK;
}

template <class OffT>
static int aggregate_typed(int64_t n, const OffT* rm, const int32_t* ent, int secondary, int32_t* labels, int64_t* num_aggregates, int64_t* stats,
                           hipStream_t st) {
  const char* who = "kkamd_graph_mis2_aggregate";
  Mis2<OffT> m;
  int rc = m.setup(who, n, rm, ent, st, 0, 4 * Mis2<OffT>::padded(sizeof(int32_t) * (size_t)n) + Mis2<OffT>::padded((size_t)n));
  if (rc) return rc;
  int32_t *set = m.template take<int32_t>((size_t)n), *old = m.template take<int32_t>((size_t)n), *con = m.template take<int32_t>((size_t)n),
          *sizes = m.template take<int32_t>((size_t)n);
  int8_t* roots = m.template take<int8_t>((size_t)n);
  if (!roots) return fail(KKAMD_ERR_STATE, "%s: the scratch is too small (internal error)", who);
  const int lanes = m.lanes, shift = m.shift, group = m.group;  // copies for the launches: the scratch holder does not copy
  unsigned long long* ctr = m.ctr;
  KK_HIP(hipMemsetAsync(labels, 0xFF, sizeof(int32_t) * (size_t)n, st));
  KK_HIP(hipMemsetAsync(roots, 0, (size_t)n, st));
  KK_HIP(hipMemsetAsync(sizes, 0, sizeof(int32_t) * (size_t)n, st));
  // phase 1
  int64_t r1 = 0, r2 = 0, primary = 0, cands = 0;
  if ((rc = m.run(who, 0, nullptr, set, &r1, &primary))) return rc;
  if (primary > 0) {
    KK_LAUNCH((mis2_phase1_kernel<OffT>), (unsigned)ceil_div(primary, group), kBlock, 0, st, primary, lanes, shift, (const int32_t*)set, n, rm, ent, labels, roots);
    KK_LAUNCH_CHECK();
    ++m.launches;
  }
  // phase 2
  bool chose = false;
  if (secondary) {
    if ((rc = m.run(who, 0, labels, set, &r2, &cands))) return rc;
    if (cands > 0) {
      const int64_t nb = ceil_div(cands, group);
      int64_t* cnt = m.counts;
      int32_t* tp  = m.tmp;
      KK_LAUNCH((mis2_cand_kernel<OffT>), (unsigned)nb, kBlock, 0, st, cands, lanes, shift, (const int32_t*)set, n, rm, ent, (const int32_t*)labels, tp, cnt);
      KK_HIP(hipMemsetAsync(cnt + nb, 0, sizeof(int64_t), st));
      ++m.launches;
      if ((rc = m.scan(nb + 1))) return rc;
      KK_LAUNCH((mis2_phase2_kernel<OffT>), (unsigned)ceil_div(nb * group, kBlock), kBlock, 0, st, nb, 8 - shift, (const int64_t*)cnt, (const int32_t*)tp, primary, n,
                rm, ent, labels, roots, ctr);
      KK_LAUNCH_CHECK();
      ++m.launches;
      chose = true;
    }
  }
  // phase 3
  KK_LAUNCH((mis2_connect_kernel<OffT>), (unsigned)ceil_div(n, group), kBlock, 0, st, n, lanes, shift, rm, ent, (const int32_t*)labels, old, con, sizes, ctr);
  KK_LAUNCH((mis2_assign_kernel<OffT>), (unsigned)ceil_div(n, kBlock), kBlock, 0, st, n, rm, ent, (const int32_t*)old, (const int32_t*)con, (const int32_t*)sizes,
            (const int8_t*)roots, labels);
  KK_LAUNCH_CHECK();
  m.launches += 2;
  unsigned long long hc[kCtrCount];
  if ((rc = m.read_ctr(hc))) return rc;
  const int64_t chosen = chose ? (int64_t)hc[kCtrTotal] : 0;
  *num_aggregates = primary + chosen;
  mis2_stats(stats, r1, r2, m.syncs, m.launches, primary, chosen, (int64_t)hc[kCtrUnlabelled], m.bytes);
  return KKAMD_OK;
}

template <class OffT>
static int coarsen_typed(int64_t n, const OffT* rm, const int32_t* ent, int offset_type, const int32_t* labels, int64_t nc, int compress, OffT* coarse_rm,
                         int32_t* coarse_ent, int64_t capacity, int64_t* coarse_nnz, int32_t* inv_off_out, int32_t* inv_lab_out, hipStream_t st) {
  const char* who = "kkamd_graph_explicit_coarsen";
  kkamd_stream_t kst = reinterpret_cast<kkamd_stream_t>(st);
  // two allocations besides the counters: the pieces whose sizes are known up front, and (with compress) the uncompressed entries
  DevBuf ctr_b, ent_b;
  Mis2Slab slab;
  KK_HIP(ctr_b.alloc(sizeof(unsigned long long) * kCtrCount));
  unsigned long long* ctr = ctr_b.as<unsigned long long>();
  unsigned long long hc[kCtrCount];
  int64_t nnz = 0;
  int rc = mis2_validate<OffT>(who, n, rm, ent, 0, ctr, st, hc, &nnz);
  if (rc) return rc;
  const size_t n_off = (size_t)(nc + 1);
  KK_HIP(slab.alloc(2 * Mis2Slab::padded(sizeof(int32_t) * n_off) + Mis2Slab::padded(sizeof(int32_t) * (size_t)n) +
                    Mis2Slab::padded(sizeof(OffT) * (size_t)(n + 1)) + 2 * Mis2Slab::padded(sizeof(OffT) * n_off)));
  int32_t *inv_off = slab.take<int32_t>(n_off), *cursor = slab.take<int32_t>(n_off), *verts = slab.take<int32_t>((size_t)n);
  OffT *start = slab.take<OffT>((size_t)(n + 1)), *raw_rm = slab.take<OffT>(n_off), *merged_rm = slab.take<OffT>(n_off);
  if (!merged_rm) return fail(KKAMD_ERR_STATE, "%s: the scratch is too small (internal error)", who);
  KK_HIP(hipMemsetAsync(inv_off, 0, sizeof(int32_t) * n_off, st));
  KK_LAUNCH(coarsen_labels_kernel, (unsigned)ceil_div(n, kBlock), kBlock, 0, st, n, labels, nc, inv_off, ctr);
  KK_LAUNCH_CHECK();
  KK_HIP(hipMemcpyAsync(hc, ctr, sizeof hc, hipMemcpyDeviceToHost, st));
  KK_HIP(hipStreamSynchronize(st));
  if (hc[kCtrBad] != kMisNoError)
    return fail(KKAMD_ERR_INVALID_ARG, "%s: vertex %lld: its label is outside [0, %lld)", who, (long long)hc[kCtrBad], (long long)nc);
  const int lanes = mis2_lane_rule(nnz, n), shift = mis2_log2(lanes);
  // the inverse map: vertices grouped by cluster, ascending inside a cluster
  if ((rc = kkamd_exclusive_scan(inv_off, nc + 1, KKAMD_I32, kst))) return rc;
  KK_HIP(hipMemcpyAsync(cursor, inv_off, sizeof(int32_t) * (size_t)(nc + 1), hipMemcpyDeviceToDevice, st));
  KK_LAUNCH(coarsen_scatter_kernel, (unsigned)ceil_div(n, kBlock), kBlock, 0, st, n, labels, cursor, verts);
  KK_LAUNCH_CHECK();
  if ((rc = kkamd_sort_crs(nc, inv_off, verts, nullptr, KKAMD_I32, KKAMD_F64, kst))) return rc;
  // where every vertex's cross-cluster entries go
  KK_LAUNCH((coarsen_count_kernel<OffT>), (unsigned)ceil_div((n + 1) * lanes, kBlock), kBlock, 0, st, n, lanes, shift, (const int32_t*)verts, rm, ent, labels, start);
  KK_LAUNCH_CHECK();
  if ((rc = kkamd_exclusive_scan(start, n + 1, offset_type, kst))) return rc;
  KK_LAUNCH((coarsen_rowmap_kernel<OffT>), (unsigned)ceil_div(nc + 1, kBlock), kBlock, 0, st, nc, (const int32_t*)inv_off, (const OffT*)start, raw_rm);
  KK_LAUNCH_CHECK();
  OffT h_total = 0;
  KK_HIP(hipMemcpyAsync(&h_total, start + n, sizeof(OffT), hipMemcpyDeviceToHost, st));
  KK_HIP(hipStreamSynchronize(st));
  const int64_t total = (int64_t)h_total;
  int64_t out_nnz = total;
  if (!compress) {
    *coarse_nnz = total;
    if (capacity < total) return fail(KKAMD_ERR_INVALID_ARG, "%s: capacity %lld is below the %lld entries of the coarse graph", who, (long long)capacity, (long long)total);
    if (total > 0) KK_LAUNCH((coarsen_fill_kernel<OffT>), (unsigned)ceil_div(n, kBlock), kBlock, 0, st, n, (const int32_t*)verts, rm, ent, labels, (const OffT*)start, coarse_ent);
    KK_LAUNCH_CHECK();
    KK_HIP(hipMemcpyAsync(coarse_rm, raw_rm, sizeof(OffT) * (size_t)(nc + 1), hipMemcpyDeviceToDevice, st));
  } else if (total == 0) {
    *coarse_nnz = 0;
    KK_HIP(hipMemsetAsync(coarse_rm, 0, sizeof(OffT) * (size_t)(nc + 1), st));
  } else {
    KK_HIP(ent_b.alloc(sizeof(int32_t) * (size_t)total));
    int32_t* raw_ent = ent_b.as<int32_t>();
    KK_LAUNCH((coarsen_fill_kernel<OffT>), (unsigned)ceil_div(n, kBlock), kBlock, 0, st, n, (const int32_t*)verts, rm, ent, labels, (const OffT*)start, raw_ent);
    KK_LAUNCH_CHECK();
    if ((rc = kkamd_sort_and_merge(nc, raw_rm, raw_ent, nullptr, offset_type, KKAMD_F64, merged_rm, nullptr, nullptr, &out_nnz, kst))) return rc;
    *coarse_nnz = out_nnz;
    if (capacity < out_nnz) return fail(KKAMD_ERR_INVALID_ARG, "%s: capacity %lld is below the %lld entries of the coarse graph", who, (long long)capacity, (long long)out_nnz);
    if ((rc = kkamd_sort_and_merge(nc, raw_rm, raw_ent, nullptr, offset_type, KKAMD_F64, merged_rm, coarse_ent, nullptr, &out_nnz, kst))) return rc;
    KK_HIP(hipMemcpyAsync(coarse_rm, merged_rm, sizeof(OffT) * (size_t)(nc + 1), hipMemcpyDeviceToDevice, st));
  }
  if (inv_off_out) KK_HIP(hipMemcpyAsync(inv_off_out, inv_off, sizeof(int32_t) * (size_t)(nc + 1), hipMemcpyDeviceToDevice, st));
  if (inv_lab_out) KK_HIP(hipMemcpyAsync(inv_lab_out, verts, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
  KK_HIP(hipStreamSynchronize(st));
  return KKAMD_OK;
}

static int mis2_check_graph(const char* who, int64_t n, const void* rm, int offset_type, const int32_t* ent) {
  if (n < 0 || n >= (int64_t)INT32_MAX) return fail(KKAMD_ERR_INVALID_ARG, "%s: num_verts %lld is outside [0, 2^31 - 1)", who, (long long)n);
  if (offset_type != KKAMD_I32 && offset_type != KKAMD_I64) return fail(KKAMD_ERR_INVALID_ARG, "%s: unknown offset_type %d", who, offset_type);
  if (n > 0 && (!rm || !ent)) return fail(KKAMD_ERR_INVALID_ARG, "%s: null pointer", who);
  return KKAMD_OK;
}

}  // namespace kk

extern "C" {

int kkamd_graph_d2_mis(int64_t num_verts, const void* d_row_map, int offset_type, const int32_t* d_entries, int algorithm, int32_t* d_mis,
                       int64_t* num_in_set, int64_t* stats, kkamd_stream_t stream) {
  const int rc = kk::mis2_check_graph("kkamd_graph_d2_mis", num_verts, d_row_map, offset_type, d_entries);
  if (rc) return rc;
  if (algorithm != KKAMD_MIS2_QUALITY && algorithm != KKAMD_MIS2_FAST) return kk::fail(KKAMD_ERR_INVALID_ARG, "graph_d2_mis: invalid algorithm");
  if (!num_in_set || (num_verts > 0 && !d_mis)) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_graph_d2_mis: null output");
  *num_in_set = 0;
  kk::mis2_stats(stats, 0, 0, 0, 0, 0, 0, 0, 0);
  if (num_verts == 0) return KKAMD_OK;
  kk::TraceRange range("KokkosGraph::graph_d2_mis[TPL_KKAMD]");
  hipStream_t st = kk::to_hip(stream);
  return offset_type == KKAMD_I64 ? kk::d2_mis_typed<int64_t>(num_verts, (const int64_t*)d_row_map, d_entries, algorithm, d_mis, num_in_set, stats, st)
                                  : kk::d2_mis_typed<int32_t>(num_verts, (const int32_t*)d_row_map, d_entries, algorithm, d_mis, num_in_set, stats, st);
}

int kkamd_graph_mis2_aggregate(int64_t num_verts, const void* d_row_map, int offset_type, const int32_t* d_entries, int secondary, int32_t* d_labels,
                               int64_t* num_aggregates, int64_t* stats, kkamd_stream_t stream) {
  const int rc = kk::mis2_check_graph("kkamd_graph_mis2_aggregate", num_verts, d_row_map, offset_type, d_entries);
  if (rc) return rc;
  if (!num_aggregates || (num_verts > 0 && !d_labels)) return kk::fail(KKAMD_ERR_INVALID_ARG, "kkamd_graph_mis2_aggregate: null output");
  *num_aggregates = 0;
  kk::mis2_stats(stats, 0, 0, 0, 0, 0, 0, 0, 0);
  if (num_verts == 0) return KKAMD_OK;
  kk::TraceRange range(secondary ? "KokkosGraph::graph_mis2_aggregate[TPL_KKAMD]" : "KokkosGraph::graph_mis2_coarsen[TPL_KKAMD]");
  hipStream_t st = kk::to_hip(stream);
  return offset_type == KKAMD_I64
             ? kk::aggregate_typed<int64_t>(num_verts, (const int64_t*)d_row_map, d_entries, secondary != 0, d_labels, num_aggregates, stats, st)
             : kk::aggregate_typed<int32_t>(num_verts, (const int32_t*)d_row_map, d_entries, secondary != 0, d_labels, num_aggregates, stats, st);
}

int kkamd_graph_explicit_coarsen(int64_t num_verts, const void* d_row_map, int offset_type, const int32_t* d_entries, const int32_t* d_labels,
                                 int64_t num_coarse, int compress, void* d_coarse_row_map, int32_t* d_coarse_entries, int64_t capacity,
                                 int64_t* coarse_nnz, int32_t* d_inverse_offsets, int32_t* d_inverse_labels, kkamd_stream_t stream) {
  const char* who = "kkamd_graph_explicit_coarsen";
  const int rc = kk::mis2_check_graph(who, num_verts, d_row_map, offset_type, d_entries);
  if (rc) return rc;
  if (num_coarse < 0 || num_coarse >= (int64_t)INT32_MAX) return kk::fail(KKAMD_ERR_INVALID_ARG, "%s: num_coarse %lld is outside [0, 2^31 - 1)", who, (long long)num_coarse);
  if (capacity < 0) return kk::fail(KKAMD_ERR_INVALID_ARG, "%s: capacity %lld is negative", who, (long long)capacity);
  if (!coarse_nnz || !d_coarse_row_map || (num_verts > 0 && !d_labels) || (capacity > 0 && !d_coarse_entries))
    return kk::fail(KKAMD_ERR_INVALID_ARG, "%s: null pointer", who);
  *coarse_nnz = 0;
  hipStream_t st = kk::to_hip(stream);
  const size_t osz = offset_type == KKAMD_I64 ? 8 : 4;
  if (num_verts == 0) {                                      // no vertex, no edge: num_coarse empty rows
    KK_HIP(hipMemsetAsync(d_coarse_row_map, 0, osz * (size_t)(num_coarse + 1), st));
    if (d_inverse_offsets) KK_HIP(hipMemsetAsync(d_inverse_offsets, 0, sizeof(int32_t) * (size_t)(num_coarse + 1), st));
    KK_HIP(hipStreamSynchronize(st));
    return KKAMD_OK;
  }
  kk::TraceRange range("KokkosGraph::graph_explicit_coarsen[TPL_KKAMD]");
  return offset_type == KKAMD_I64
             ? kk::coarsen_typed<int64_t>(num_verts, (const int64_t*)d_row_map, d_entries, offset_type, d_labels, num_coarse, compress != 0,
                                          (int64_t*)d_coarse_row_map, d_coarse_entries, capacity, coarse_nnz, d_inverse_offsets, d_inverse_labels, st)
             : kk::coarsen_typed<int32_t>(num_verts, (const int32_t*)d_row_map, d_entries, offset_type, d_labels, num_coarse, compress != 0,
                                          (int32_t*)d_coarse_row_map, d_coarse_entries, capacity, coarse_nnz, d_inverse_offsets, d_inverse_labels, st);
}

}  // extern "C"
