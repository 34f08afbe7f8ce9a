// kk_levels.h -- the level schedule the level-scheduled routines share (kk_sptrsv.hip, kk_spiluk.hip): the rows of a triangle grouped by
// level on the device, the three launch knobs, and the launches of one sweep over the levels.  The analysis is in kk_sptrsv.hip.
#pragma once
#include "kk_common.h"
#include <vector>

namespace kk {

struct LevelLaunch {
  int first, nlev;      // levels covered
  int lpr, chain;       // lanes per row; 1: one single-workgroup launch over the nlev levels
};

// A plain struct the handles hold by value; clear() before the handle is deleted.
struct LevelSchedule {
  int lanes_per_row = 0, chain_rows = 64, chain_levels = 1024;   // the knobs
  int32_t* d_grouped = nullptr;                          // the rows level by level, ascending inside a level
  int64_t* d_level_off = nullptr;
  std::vector<int64_t> level_off, level_entries;        // host: num_levels + 1 offsets into the grouped list, entries per level
  std::vector<LevelLaunch> plan;                         // the launches of one sweep
  int64_t max_level_rows = 0, chain_launches = 0, chained_levels = 0;

  int64_t num_levels() const { return level_off.empty() ? 0 : (int64_t)level_off.size() - 1; }
  // back to the unanalysed state; the knobs stay
  void clear() {
    if (d_grouped) (void)hipFree(d_grouped);
    if (d_level_off) (void)hipFree(d_level_off);
    d_grouped = nullptr;
    d_level_off = nullptr;
    level_off.clear(); level_entries.clear(); plan.clear();
    max_level_rows = chain_launches = chained_levels = 0;
  }
};

inline int log2i(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }

// the smallest power of two, 1..64, that covers a mean row length: one pass over an average row
inline int pow2_covering(int64_t mean) {
  int lpr = 1;
  while (lpr < kWave && lpr < mean) lpr *= 2;
  return lpr;
}

// The level sets of the n x n triangle (row_map, entries) with its diagonal stored, on the device (kk_sptrsv.hip, the four steps of
// its header): fills the device arrays, level_off, level_entries and max_level_rows of a cleared schedule and hands back level_list
// (1-based) and the diagonal's position inside every row.  n == 0 gives no level and no device array.  A failure leaves the
// schedule as it was; the error texts name kkamd_sptrsv_symbolic, the entry point this analysis belongs to.  It stays in that unit,
// so a library with kk_spiluk.hip links kk_sptrsv.hip too, as it always has.
int analyse_levels(LevelSchedule* s, int64_t n, int lower, const void* row_map, const int32_t* entries, int offset_type, hipStream_t st,
                   DevBuf* level_list, DevBuf* diagpos);

// "lanes_per_row", "chain_rows", "chain_levels" with their ranges; who is the C function the error texts name
inline int set_knob(LevelSchedule* s, const char* who, const char* key, int value) {
  const std::string k(key);
  if (k == "lanes_per_row") {
    if (value < 0 || value > kWave || (value & (value - 1))) return fail(KKAMD_ERR_INVALID_ARG, "%s: lanes_per_row %d is not 0 or a power of two up to 64", who, value);
    s->lanes_per_row = value;
  } else if (k == "chain_rows") {
    if (value < 0) return fail(KKAMD_ERR_INVALID_ARG, "%s: chain_rows %d is negative", who, value);
    s->chain_rows = value;
  } else if (k == "chain_levels") {
    if (value < 1) return fail(KKAMD_ERR_INVALID_ARG, "%s: chain_levels %d is below 1", who, value);
    s->chain_levels = value;
  } else {
    return fail(KKAMD_ERR_INVALID_ARG, "%s: unknown key '%s'", who, key);
  }
  return KKAMD_OK;
}

// the read-only keys every level-scheduled handle serves; false when key is none of them
inline bool get_common(const LevelSchedule& s, const std::string& k, int64_t* value) {
  if (k == "num_levels") *value = s.num_levels();
  else if (k == "max_level_rows") *value = s.max_level_rows;
  else if (k == "launches") *value = (int64_t)s.plan.size();
  else if (k == "chain_launches") *value = s.chain_launches;
  else if (k == "chained_levels") *value = s.chained_levels;
  else if (k == "lanes_per_row") *value = s.lanes_per_row;
  else if (k == "chain_rows") *value = s.chain_rows;
  else if (k == "chain_levels") *value = s.chain_levels;
  else return false;
  return true;
}

// The launches of one sweep from the level sizes and the knobs: one per level, except that, with chaining, every run of two or more
// consecutive levels with at most chain_rows rows each goes into ceil(run / chain_levels) chain launches.
// lanes(entries, rows) gives the lanes per row of a launch that covers that many entries in that many rows.
template <class Lanes>
void build_plan(LevelSchedule* s, bool chaining, Lanes lanes) {
  s->plan.clear();
  s->chain_launches = s->chained_levels = 0;
  const std::vector<int64_t>& off = s->level_off;
  const int64_t L = s->num_levels();
  int64_t l = 0;
  while (l < L) {
    int64_t run = 0;
    if (chaining)
      while (l + run < L && off[l + run + 1] - off[l + run] <= s->chain_rows) ++run;
    if (run < 2) {
      s->plan.push_back({(int)l, 1, lanes(s->level_entries[l], off[l + 1] - off[l]), 0});
      ++l;
      continue;
    }
    for (int64_t p = 0; p < run; p += s->chain_levels) {
      const int64_t nl = run - p < s->chain_levels ? run - p : s->chain_levels;
      int64_t entries = 0;
      for (int64_t q = l + p; q < l + p + nl; ++q) entries += s->level_entries[q];
      s->plan.push_back({(int)(l + p), (int)nl, lanes(entries, off[l + p + nl] - off[l + p]), 1});
      s->chain_launches += 1;
      s->chained_levels += nl;
    }
    l += run;
  }
}

}  // namespace kk
