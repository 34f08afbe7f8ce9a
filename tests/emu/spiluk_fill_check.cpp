// TEST INFRASTRUCTURE: the host side of kkamd_spiluk_symbolic (kk_spiluk_fill.h: validation and the ILU(k) fill loop) as a stand-alone
// program, so that it can run under the host sanitizers (spiluk.mk builds it with -fsanitize=address,undefined).  It feeds the loop
// the malformed graphs the library must refuse before it indexes anything by them, and a few good ones whose fill is known.
#include "kk_spiluk_fill.h"
#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

template <class OffT>
static int run(int64_t n, std::vector<OffT> rm, std::vector<int32_t> ent, int fill_lev, kk::IlukPattern* out, int64_t* bad) {
  *bad = -1;
  if (int k = kk::iluk_check_row_map<OffT>(n, rm.data(), bad)) return k;
  // exactly rm[n] entries are handed over: a read past them is a heap overflow the sanitizer reports
  std::vector<int32_t> exact(ent.begin(), ent.begin() + (size_t)rm[(size_t)n]);
  if (int k = kk::iluk_check_entries<OffT>(n, rm.data(), exact.data(), bad)) return k;
  kk::iluk_fill<OffT>(n, rm.data(), exact.data(), fill_lev, out);
  return kk::kFillOk;
}

template <class OffT>
static void all() {
  kk::IlukPattern p;
  int64_t bad;
  // row map: descending, negative start
  EXPECT(run<OffT>(3, {0, 2, 1, 3}, {0, 1, 1, 2}, 0, &p, &bad) == kk::kFillRowMap && bad == 1);
  EXPECT(run<OffT>(2, {-1, 1, 2}, {0, 1, 1}, 0, &p, &bad) == kk::kFillRowMap && bad == 0);
  // columns: past the end, negative, far out
  EXPECT(run<OffT>(3, {0, 1, 3, 4}, {0, 1, 3, 2}, 1, &p, &bad) == kk::kFillColumn && bad == 1);
  EXPECT(run<OffT>(3, {0, 1, 3, 4}, {0, 1, -1, 2}, 1, &p, &bad) == kk::kFillColumn && bad == 1);
  EXPECT(run<OffT>(3, {0, 1, 2, 4}, {0, 1, 2, 2147483647}, 1, &p, &bad) == kk::kFillColumn && bad == 2);
  // a repeated column, off the diagonal and on it; the first offending row is named
  EXPECT(run<OffT>(3, {0, 1, 4, 7}, {0, 0, 1, 0, 2, 2, 1}, 2, &p, &bad) == kk::kFillRepeat && bad == 1);
  EXPECT(run<OffT>(3, {0, 2, 3, 4}, {0, 0, 1, 2}, 2, &p, &bad) == kk::kFillRepeat && bad == 0);
  // n = 0, n = 1 with and without a diagonal, an empty row
  EXPECT(run<OffT>(0, {0}, {}, 0, &p, &bad) == kk::kFillOk && p.L_ent.empty() && p.U_ent.empty() && p.L_rm.size() == 1);
  EXPECT(run<OffT>(1, {0, 1}, {0}, 3, &p, &bad) == kk::kFillOk && p.L_ent == std::vector<int32_t>{0} && p.U_ent == std::vector<int32_t>{0});
  EXPECT(run<OffT>(1, {0, 0}, {}, 3, &p, &bad) == kk::kFillOk && p.L_ent == std::vector<int32_t>{0} && p.U_ent == std::vector<int32_t>{0});
  // the arrow matrix pointing up-left (row 0 and column 0 full, shuffled rows): ILU(0) keeps the pattern, ILU(1) fills everything
  const int64_t n = 5;
  std::vector<OffT> rm = {0, 5, 7, 9, 11, 13};
  std::vector<int32_t> ent = {3, 0, 4, 1, 2, 1, 0, 0, 2, 3, 0, 0, 4};
  EXPECT(run<OffT>(n, rm, ent, 0, &p, &bad) == kk::kFillOk && p.L_ent.size() == 9 && p.U_ent.size() == 9);
  EXPECT((p.U_ent == std::vector<int32_t>{0, 1, 2, 3, 4, 1, 2, 3, 4}) && (p.L_ent == std::vector<int32_t>{0, 0, 1, 0, 2, 0, 3, 0, 4}));
  EXPECT(run<OffT>(n, rm, ent, 1, &p, &bad) == kk::kFillOk && p.L_ent.size() == 15 && p.U_ent.size() == 15);
  EXPECT((p.L_rm == std::vector<int64_t>{0, 1, 3, 6, 10, 15}) && (p.U_rm == std::vector<int64_t>{0, 5, 9, 12, 14, 15}));
  // the sum rule: in the chain 1 <- 0, 2 <- 1, 3 <- 2 with (0,3) stored, (1,3) has level 1, (2,3) level 2
  rm = {0, 2, 4, 6, 8};
  ent = {0, 3, 0, 1, 1, 2, 2, 3};
  EXPECT(run<OffT>(4, rm, ent, 0, &p, &bad) == kk::kFillOk && p.U_ent.size() == 5);
  EXPECT(run<OffT>(4, rm, ent, 1, &p, &bad) == kk::kFillOk && p.U_ent.size() == 6);
  EXPECT(run<OffT>(4, rm, ent, 2, &p, &bad) == kk::kFillOk && p.U_ent.size() == 7 && (p.U_ent == std::vector<int32_t>{0, 3, 1, 3, 2, 3, 3}));
}

int main() {
  all<int32_t>();
  all<int64_t>();
  if (failures) return 1;
  std::printf("spiluk_fill_check: all passed\n");
  return 0;
}
