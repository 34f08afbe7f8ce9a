// kk_spiluk_fill.h -- the host side of kkamd_spiluk_symbolic: validation of the caller's graph and the ILU(k) fill computation.
// Plain C++ (no HIP), so that a stand-alone program can run it under the host sanitizers (tools/spiluk_fill_check.cpp).
//
// The fill rule is the reference's loop (sparse/impl/KokkosSparse_spiluk_symbolic_impl.hpp:282-389): entries of A have level 0;
// eliminating row i by pivot j, pivots in ascending column order, gives column c of U row j the level lev(i,j) + lev(j,c) + 1, kept
// when that is <= fill_lev; an entry already present takes the minimum.  The reference finds the next pivot by a linear search
// for the smallest remaining column (:184-210); a heap gives the same order.  Rows leave sorted by column -- L: columns < i, then
// the unit diagonal; U: the diagonal, present even when A has none, then columns > i -- as sort_crs_graph leaves them (:395-398).
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

namespace kk {

enum { kFillOk = 0, kFillRowMap = 1, kFillColumn = 2, kFillRepeat = 3 };

// the row map alone: nothing else may be read before it is known to be ascending from a non-negative start
template <class OffT>
inline int iluk_check_row_map(int64_t n, const OffT* rm, int64_t* bad_row) {
  if (n > 0 && (int64_t)rm[0] < 0) { *bad_row = 0; return kFillRowMap; }
  for (int64_t i = 0; i < n; ++i)
    if ((int64_t)rm[i + 1] < (int64_t)rm[i]) { *bad_row = i; return kFillRowMap; }
  return kFillOk;
}

// every column in [0, n) and no column twice in a row; the first offending row is named.  stamp is indexed by checked columns only
template <class OffT>
inline int iluk_check_entries(int64_t n, const OffT* rm, const int32_t* ent, int64_t* bad_row) {
  std::vector<int64_t> stamp((size_t)n, -1);
  for (int64_t i = 0; i < n; ++i)
    for (int64_t p = (int64_t)rm[i]; p < (int64_t)rm[i + 1]; ++p) {
      const int64_t c = ent[p];
      if (c < 0 || c >= n) { *bad_row = i; return kFillColumn; }
      if (stamp[(size_t)c] == i) { *bad_row = i; return kFillRepeat; }
      stamp[(size_t)c] = i;
    }
  return kFillOk;
}

struct IlukPattern {
  std::vector<int64_t> L_rm, U_rm;
  std::vector<int32_t> L_ent, U_ent;
};

// the graph must have passed both checks
template <class OffT>
inline void iluk_fill(int64_t n, const OffT* rm, const int32_t* ent, int fill_lev, IlukPattern* out) {
  out->L_rm.assign((size_t)n + 1, 0);
  out->U_rm.assign((size_t)n + 1, 0);
  out->L_ent.clear();
  out->U_ent.clear();
  std::vector<int32_t> U_lev;                                   // level of every entry of U, beside U_ent
  std::vector<int32_t> iw((size_t)n, -1);                       // column -> position in the row's L or U list
  std::vector<std::pair<int32_t, int32_t>> Lr, Ur;              // (column, level) of the row under way
  std::priority_queue<int32_t, std::vector<int32_t>, std::greater<int32_t>> pivots;
  for (int64_t i = 0; i < n; ++i) {
    Lr.clear();
    Ur.clear();
    for (int64_t p = (int64_t)rm[i]; p < (int64_t)rm[i + 1]; ++p) {
      const int32_t c = ent[p];
      if (c > i) { iw[(size_t)c] = (int32_t)Ur.size(); Ur.push_back({c, 0}); }
      else if (c < i) { iw[(size_t)c] = (int32_t)Lr.size(); Lr.push_back({c, 0}); pivots.push(c); }
    }
    while (!pivots.empty()) {
      const int32_t j = pivots.top();
      pivots.pop();
      const int32_t jlev = Lr[(size_t)iw[(size_t)j]].second;
      for (int64_t k = out->U_rm[(size_t)j] + 1; k < out->U_rm[(size_t)j + 1]; ++k) {
        const int32_t c = out->U_ent[(size_t)k];
        const int64_t lev1 = (int64_t)jlev + U_lev[(size_t)k] + 1;
        if (lev1 > fill_lev) continue;
        const int32_t pos = iw[(size_t)c];
        if (pos == -1) {                                        // fill-in; c > j, so a new pivot comes after the current one
          if (c > i) { iw[(size_t)c] = (int32_t)Ur.size(); Ur.push_back({c, (int32_t)lev1}); }
          else if (c < i) { iw[(size_t)c] = (int32_t)Lr.size(); Lr.push_back({c, (int32_t)lev1}); pivots.push(c); }
        } else if (c > i) {
          Ur[(size_t)pos].second = std::min(Ur[(size_t)pos].second, (int32_t)lev1);
        } else if (c < i) {
          Lr[(size_t)pos].second = std::min(Lr[(size_t)pos].second, (int32_t)lev1);
        }
      }
    }
    for (const auto& e : Lr) iw[(size_t)e.first] = -1;
    for (const auto& e : Ur) iw[(size_t)e.first] = -1;
    std::sort(Lr.begin(), Lr.end());
    std::sort(Ur.begin(), Ur.end());
    out->U_ent.push_back((int32_t)i);
    U_lev.push_back(0);
    for (const auto& e : Ur) { out->U_ent.push_back(e.first); U_lev.push_back(e.second); }
    out->U_rm[(size_t)i + 1] = (int64_t)out->U_ent.size();
    for (const auto& e : Lr) out->L_ent.push_back(e.first);
    out->L_ent.push_back((int32_t)i);
    out->L_rm[(size_t)i + 1] = (int64_t)out->L_ent.size();
  }
}

}  // namespace kk
