// Host-side test of the sparse triangular solve's drop-in headers (run on the GPU by tests/test_gpu_sptrsv_host_api.py):
// KokkosSparse::sptrsv_symbolic / sptrsv_solve through KokkosKernelsHandle::create_sptrsv_handle, with and without an execution
// space instance, under the KokkosSparse::Experimental:: names too, for (double, int offsets) and (float, size_t offsets).
// The cases are built here: a random lower triangle and its transpose with entries in shuffled order, integer off-diagonals with
// 1 <= |a| <= 4, diagonals from {0.5, 1, 2, 4, -1, -2}, a known integer solution x* in [-8, 8] and b = A x* -- every partial sum is a
// small integer, so every order of summation gives x* exactly and the results are compared with ==.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>
#include "KokkosSparse_sptrsv.hpp"

#pragma GCC diagnostic ignored "-Wdeprecated-declarations"   // the Experimental:: names are deprecated on purpose, as in the reference

using device = Kokkos::Device<Kokkos::HIP, Kokkos::HIPSpace>;
using KokkosSparse::Experimental::SPTRSVAlgorithm;
static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

template <class scalar, class size_type> struct Triangle {
  int n = 0;
  std::vector<size_type> rm;
  std::vector<int> ent;
  std::vector<scalar> val, b, xstar;
};

// lower: row i holds up to max_off entries from the earlier rows (repetitions allowed) and its diagonal; upper: the transpose
template <class scalar, class size_type>
Triangle<scalar, size_type> make_triangle(int n, int max_off, bool lower, unsigned seed) {
  std::mt19937 g(seed);
  std::vector<std::vector<std::pair<int, scalar>>> rows(n);
  const scalar diag[6] = {(scalar)0.5, 1, 2, 4, -1, -2};
  for (int i = 0; i < n; ++i) {
    const int cnt = i ? (int)(g() % (unsigned)(std::min(max_off, i) + 1)) : 0;
    for (int q = 0; q < cnt; ++q) {
      const int j = (int)(g() % (unsigned)i);
      const scalar a = (scalar)((int)(g() % 4) + 1) * ((g() & 1) ? 1 : -1);
      if (lower) rows[i].push_back({j, a}); else rows[j].push_back({i, a});
    }
    rows[i].push_back({i, diag[g() % 6]});
  }
  Triangle<scalar, size_type> t;
  t.n = n; t.rm.assign(n + 1, 0); t.xstar.resize(n); t.b.assign(n, 0);
  for (int i = 0; i < n; ++i) t.xstar[i] = (scalar)((int)(g() % 17) - 8);
  for (int i = 0; i < n; ++i) {
    std::shuffle(rows[i].begin(), rows[i].end(), g);
    for (auto& e : rows[i]) { t.ent.push_back(e.first); t.val.push_back(e.second); t.b[i] += e.second * t.xstar[e.first]; }
    t.rm[i + 1] = (size_type)t.ent.size();
  }
  return t;
}

// the reference's level definition (sparse/impl/KokkosSparse_sptrsv_symbolic_impl.hpp:194-214, :617-639), rows in solve order
template <class T> int count_levels(const T& t, bool lower) {
  std::vector<int> level(t.n, 0);
  int nlev = 0;
  for (int q = 0; q < t.n; ++q) {
    const int i = lower ? q : t.n - 1 - q;
    int l = 0;
    for (size_t p = t.rm[i]; p < (size_t)t.rm[i + 1]; ++p) if (t.ent[p] != i) l = std::max(l, level[t.ent[p]]);
    level[i] = l + 1; nlev = std::max(nlev, l + 1);
  }
  return nlev;
}

template <class scalar, class V> bool equals(const V& d_x, const std::vector<scalar>& expect) {
  auto h = Kokkos::create_mirror_view(d_x);
  Kokkos::deep_copy(h, d_x);
  for (size_t i = 0; i < expect.size(); ++i) if (!(h(i) == expect[i])) return false;
  return true;
}

template <class scalar, class size_type>
void run_case(int n, int max_off, bool lower, SPTRSVAlgorithm algo, unsigned seed) {
  using KH = KokkosKernels::Experimental::KokkosKernelsHandle<size_type, int, scalar, Kokkos::HIP, Kokkos::HIPSpace, Kokkos::HIPSpace>;
  const auto t = make_triangle<scalar, size_type>(n, max_off, lower, seed);
  Kokkos::View<size_type*, device> rm("rm", n + 1);
  Kokkos::View<int*, device> ent("ent", t.ent.size());
  Kokkos::View<scalar*, device> val("val", t.val.size()), b("b", n), x("x", n);
  Kokkos::deep_copy(rm, Kokkos::View<const size_type*, Kokkos::HostSpace>(t.rm.data(), t.rm.size()));
  Kokkos::deep_copy(ent, Kokkos::View<const int*, Kokkos::HostSpace>(t.ent.data(), t.ent.size()));
  Kokkos::deep_copy(val, Kokkos::View<const scalar*, Kokkos::HostSpace>(t.val.data(), t.val.size()));
  Kokkos::deep_copy(b, Kokkos::View<const scalar*, Kokkos::HostSpace>(t.b.data(), t.b.size()));
  const scalar nan = std::numeric_limits<scalar>::quiet_NaN();

  KH kh;
  EXPECT(kh.get_sptrsv_handle() == nullptr);
  kh.create_sptrsv_handle(algo, n, lower);
  auto* sh = kh.get_sptrsv_handle();
  EXPECT(sh->get_algorithm() == algo && (int)sh->get_nrows() == n && sh->is_lower_tri() == lower && sh->is_upper_tri() != lower);
  EXPECT(kh.is_sptrsv_lower_tri() == lower && !sh->is_symbolic_complete());
  bool threw = false;                                   // solve before symbolic: std::invalid_argument
  try { KokkosSparse::sptrsv_solve(&kh, rm, ent, val, b, x); } catch (const std::invalid_argument&) { threw = true; }
  EXPECT(threw);

  // without an execution space
  KokkosSparse::sptrsv_symbolic(&kh, rm, ent);
  EXPECT(sh->is_symbolic_complete() && (int)sh->get_num_levels() == count_levels(t, lower));
  Kokkos::deep_copy(x, nan);
  KokkosSparse::sptrsv_solve(&kh, rm, ent, val, b, x);
  Kokkos::fence();
  EXPECT(equals(x, t.xstar));

  // with an execution space instance on its own stream; const views of the matrix; the symbolic overload that takes values
  hipStream_t stream = nullptr;
  EXPECT(hipStreamCreate(&stream) == hipSuccess);
  {
    Kokkos::HIP space(stream);
    typename Kokkos::View<size_type*, device>::const_type c_rm = rm;
    typename Kokkos::View<int*, device>::const_type c_ent = ent;
    typename Kokkos::View<scalar*, device>::const_type c_val = val, c_b = b;
    KokkosSparse::sptrsv_symbolic(space, &kh, c_rm, c_ent, c_val);
    Kokkos::deep_copy(x, nan);
    KokkosSparse::sptrsv_solve(space, &kh, c_rm, c_ent, c_val, c_b, x);
    space.fence();
    EXPECT(equals(x, t.xstar));
    // the deprecated Experimental:: names forward; x aliased to b
    KokkosSparse::Experimental::sptrsv_symbolic(space, &kh, rm, ent);
    Kokkos::View<scalar*, device> xb("xb", n);
    Kokkos::deep_copy(xb, b);
    KokkosSparse::Experimental::sptrsv_solve(space, &kh, rm, ent, val, xb, xb);
    space.fence();
    EXPECT(equals(xb, t.xstar));
  }
  EXPECT(hipStreamDestroy(stream) == hipSuccess);
  KokkosSparse::Experimental::sptrsv_symbolic(&kh, rm, ent);
  Kokkos::deep_copy(x, nan);
  KokkosSparse::Experimental::sptrsv_solve(&kh, rm, ent, val, b, x);
  Kokkos::fence();
  EXPECT(equals(x, t.xstar));

  // the wrong triangle is refused by the analysis (std::runtime_error) and leaves the handle without one
  if (t.ent.size() > (size_t)n) {
    KH other;
    other.create_sptrsv_handle(algo, n, !lower);
    threw = false;
    try { KokkosSparse::sptrsv_symbolic(&other, rm, ent); } catch (const std::runtime_error&) { threw = true; }
    EXPECT(threw && !other.get_sptrsv_handle()->is_symbolic_complete());
  }
  kh.destroy_sptrsv_handle();
  EXPECT(kh.get_sptrsv_handle() == nullptr);
}

int main() {
  Kokkos::initialize();
  {
    const SPTRSVAlgorithm algos[3] = {SPTRSVAlgorithm::SEQLVLSCHD_RP, SPTRSVAlgorithm::SEQLVLSCHD_TP1, SPTRSVAlgorithm::SEQLVLSCHD_TP1CHAIN};
    unsigned seed = 1;
    for (SPTRSVAlgorithm a : algos)
      for (bool lower : {true, false}) {
        run_case<double, int>(700, 3, lower, a, seed++);          // wide levels, a narrow tail
        run_case<float, size_t>(300, 90, lower, a, seed++);       // long rows, many narrow levels
        run_case<double, size_t>(1, 0, lower, a, seed++);
        run_case<float, int>(0, 0, lower, a, seed++);
      }
    using KH = KokkosKernels::Experimental::KokkosKernelsHandle<int, int, double, Kokkos::HIP, Kokkos::HIPSpace, Kokkos::HIPSpace>;
    KH kh;
    bool threw = false;
    try { kh.create_sptrsv_handle(SPTRSVAlgorithm::SPTRSV_CUSPARSE, 4, true); } catch (const std::runtime_error&) { threw = true; }
    EXPECT(threw && kh.get_sptrsv_handle() == nullptr);
    EXPECT(KokkosSparse::Experimental::StringToSPTRSVAlgorithm("SEQLVLSCHD_TP1CHAIN") == SPTRSVAlgorithm::SEQLVLSCHD_TP1CHAIN);
    Kokkos::View<int*, device> rm("rm", 5), ent("ent", 4);
    threw = false;                                                 // no SPTRSV sub-handle: std::invalid_argument
    try { KokkosSparse::sptrsv_symbolic(&kh, rm, ent); } catch (const std::invalid_argument&) { threw = true; }
    EXPECT(threw);
  }
  Kokkos::finalize();
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("sptrsv drop-in: all passed\n");
  return 0;
}
