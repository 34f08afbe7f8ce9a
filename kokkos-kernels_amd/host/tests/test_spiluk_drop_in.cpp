// Host-side test of the ILU(k) drop-in headers (run on the GPU by tests/test_gpu_spiluk_host_api.py):
// KokkosSparse::spiluk_symbolic / spiluk_numeric through KokkosKernelsHandle::create_spiluk_handle, under the
// KokkosSparse::Experimental:: names too, for (double, int offsets) and (float, size_t offsets), at fill levels 0 and 2.
// The matrix is built here (the 9-point stencil on a small grid with a few entries removed, rows shuffled, diagonally dominant random
// values) and so are the expected factors: a dense restatement of the sum-rule fill and of the row recurrence, in the same scalar
// type.  Values are compared within 64 ulp of |v| + 1: the dense loop applies the same updates in the same order, only the
// contraction of x - f * u may differ.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <string>
#include <vector>
#include "KokkosSparse_spiluk.hpp"

#pragma GCC diagnostic ignored "-Wdeprecated-declarations"   // the Experimental:: names are deprecated on purpose, as in the reference

using device = Kokkos::Device<Kokkos::HIP, Kokkos::HIPSpace>;
using KokkosSparse::Experimental::SPILUKAlgorithm;
static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

template <class scalar, class size_type> struct Matrix {
  int n = 0;
  std::vector<size_type> rm;
  std::vector<int> ent;
  std::vector<scalar> val;
};

template <class scalar, class size_type> Matrix<scalar, size_type> make_matrix(int nx, int ny, unsigned seed) {
  std::mt19937 g(seed);
  Matrix<scalar, size_type> m;
  m.n = nx * ny;
  m.rm.assign(m.n + 1, 0);
  for (int i = 0; i < m.n; ++i) {
    std::vector<std::pair<int, scalar>> row;
    scalar sum = 0;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int x = i % nx + dx, y = i / nx + dy;
        if ((dx == 0 && dy == 0) || x < 0 || x >= nx || y < 0 || y >= ny || g() % 5 == 0) continue;
        const scalar a = (scalar)((int)(g() % 200) - 100) / (scalar)100;
        row.push_back({x + nx * y, a});
        sum += std::abs(a);
      }
    row.push_back({i, (scalar)1 + sum});
    std::shuffle(row.begin(), row.end(), g);
    for (auto& e : row) { m.ent.push_back(e.first); m.val.push_back(e.second); }
    m.rm[i + 1] = (size_type)m.ent.size();
  }
  return m;
}

// dense ILU(k): lev < 0 marks a position outside the pattern; L holds the multipliers below the diagonal, U the rest
template <class scalar> struct Dense {
  int n;
  std::vector<int> lev;
  std::vector<scalar> w;
  bool in(int i, int j) const { return lev[(size_t)i * n + j] >= 0; }
  scalar at(int i, int j) const { return w[(size_t)i * n + j]; }
};

template <class scalar, class M> Dense<scalar> dense_iluk(const M& m, int fill) {
  const int n = m.n, INF = 1 << 20;
  Dense<scalar> d{n, std::vector<int>((size_t)n * n, INF), std::vector<scalar>((size_t)n * n, 0)};
  for (int i = 0; i < n; ++i) {
    d.lev[(size_t)i * n + i] = 0;
    for (size_t p = m.rm[i]; p < (size_t)m.rm[i + 1]; ++p) { d.lev[(size_t)i * n + m.ent[p]] = 0; d.w[(size_t)i * n + m.ent[p]] = m.val[p]; }
    for (int k = 0; k < i; ++k) {
      if (d.lev[(size_t)i * n + k] > fill) continue;
      for (int j = k + 1; j < n; ++j) {
        if (j == i || d.lev[(size_t)k * n + j] > fill) continue;
        const int l1 = d.lev[(size_t)i * n + k] + d.lev[(size_t)k * n + j] + 1;
        if (l1 <= fill) d.lev[(size_t)i * n + j] = std::min(d.lev[(size_t)i * n + j], l1);
      }
    }
    for (int j = 0; j < n; ++j) if (d.lev[(size_t)i * n + j] > fill) d.lev[(size_t)i * n + j] = INF;
    scalar* w = &d.w[(size_t)i * n];
    for (int k = 0; k < i; ++k) {
      if (d.lev[(size_t)i * n + k] > fill) continue;
      const scalar f = w[k] / d.w[(size_t)k * n + k];
      w[k] = f;
      for (int j = k + 1; j < n; ++j)
        if (d.lev[(size_t)k * n + j] <= fill && d.lev[(size_t)i * n + j] <= fill) w[j] = w[j] - f * d.w[(size_t)k * n + j];
    }
    if (w[i] == (scalar)0) w[i] = (scalar)1e6;
  }
  for (int& l : d.lev) if (l > fill) l = -1;
  return d;
}

template <class V> std::vector<typename V::non_const_value_type> to_host(const V& v) {
  auto h = Kokkos::create_mirror_view(v);
  Kokkos::deep_copy(h, v);
  std::vector<typename V::non_const_value_type> out(v.extent(0));
  for (size_t i = 0; i < out.size(); ++i) out[i] = h(i);
  return out;
}

template <class scalar> bool close(scalar a, scalar b) {
  return std::abs(a - b) <= (scalar)64 * std::numeric_limits<scalar>::epsilon() * (std::abs(b) + (scalar)1);
}

template <class scalar, class size_type> void run_case(int nx, int ny, int fill, unsigned seed) {
  using KH = KokkosKernels::Experimental::KokkosKernelsHandle<size_type, int, scalar, Kokkos::HIP, Kokkos::HIPSpace, Kokkos::HIPSpace>;
  const auto m = make_matrix<scalar, size_type>(nx, ny, seed);
  const int n  = m.n;
  const auto d = dense_iluk<scalar>(m, fill);
  size_t nnzL = 0, nnzU = 0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) if (d.in(i, j)) ++(j < i ? nnzL : nnzU);
  nnzL += (size_t)n;                                         // the unit diagonal of L
  Kokkos::View<size_type*, device> A_rm("A_rm", n + 1), L_rm("L_rm", n + 1), U_rm("U_rm", n + 1);
  Kokkos::View<int*, device> A_ent("A_ent", m.ent.size());
  Kokkos::View<scalar*, device> A_val("A_val", m.val.size());
  Kokkos::deep_copy(A_rm, Kokkos::View<const size_type*, Kokkos::HostSpace>(m.rm.data(), m.rm.size()));
  Kokkos::deep_copy(A_ent, Kokkos::View<const int*, Kokkos::HostSpace>(m.ent.data(), m.ent.size()));
  Kokkos::deep_copy(A_val, Kokkos::View<const scalar*, Kokkos::HostSpace>(m.val.data(), m.val.size()));

  KH kh;
  EXPECT(kh.get_spiluk_handle() == nullptr);
  const size_t guess = 4 * m.ent.size() + (size_t)n;         // the usual way: a generous estimate, then a resize to the true counts
  kh.create_spiluk_handle(SPILUKAlgorithm::SEQLVLSCHD_TP1, n, guess, guess);
  auto* sh = kh.get_spiluk_handle();
  EXPECT(sh->get_algorithm() == SPILUKAlgorithm::SEQLVLSCHD_TP1 && (int)sh->get_nrows() == n && !sh->is_symbolic_complete());
  EXPECT((size_t)sh->get_nnzL() == guess && (size_t)sh->get_nnzU() == guess);
  Kokkos::View<int*, device> L_ent("L_ent", sh->get_nnzL()), U_ent("U_ent", sh->get_nnzU());
  Kokkos::View<scalar*, device> L_val("L_val", sh->get_nnzL()), U_val("U_val", sh->get_nnzU());
  bool threw = false;                                        // numeric before symbolic: the reference's runtime exception
  try { KokkosSparse::spiluk_numeric(&kh, fill, A_rm, A_ent, A_val, L_rm, L_ent, L_val, U_rm, U_ent, U_val); }
  catch (const std::runtime_error& e) { threw = std::string(e.what()).find("spiluk_symbolic must be called before spiluk_numeric") != std::string::npos; }
  EXPECT(threw);
  threw = false;                                             // a negative fill level
  try { KokkosSparse::spiluk_symbolic(&kh, -1, A_rm, A_ent, L_rm, L_ent, U_rm, U_ent); }
  catch (const std::runtime_error& e) { threw = std::string(e.what()).find("fill_lev: -1. Valid value is >= 0.") != std::string::npos; }
  EXPECT(threw);

  KokkosSparse::spiluk_symbolic(&kh, fill, A_rm, A_ent, L_rm, L_ent, U_rm, U_ent);
  EXPECT(sh->is_symbolic_complete() && (size_t)sh->get_nnzL() == nnzL && (size_t)sh->get_nnzU() == nnzU);
  EXPECT(sh->get_num_levels() >= 1 && (int)sh->get_num_levels() <= n && sh->get_level_maxrows() >= 1);
  // the resize after symbolic: views of exactly get_nnzL() / get_nnzU() entries, the graphs copied over
  Kokkos::View<int*, device> L_ent2("L_ent2", sh->get_nnzL()), U_ent2("U_ent2", sh->get_nnzU());
  Kokkos::View<scalar*, device> L_val2("L_val2", sh->get_nnzL()), U_val2("U_val2", sh->get_nnzU());
  Kokkos::deep_copy(L_ent2, Kokkos::subview(L_ent, std::make_pair(0, (int)sh->get_nnzL())));
  Kokkos::deep_copy(U_ent2, Kokkos::subview(U_ent, std::make_pair(0, (int)sh->get_nnzU())));
  Kokkos::deep_copy(L_val2, std::numeric_limits<scalar>::quiet_NaN());
  Kokkos::deep_copy(U_val2, std::numeric_limits<scalar>::quiet_NaN());
  KokkosSparse::spiluk_numeric(&kh, fill, A_rm, A_ent, A_val, L_rm, L_ent2, L_val2, U_rm, U_ent2, U_val2);
  Kokkos::fence();

  auto check = [&](const Kokkos::View<scalar*, device>& Lv, const Kokkos::View<scalar*, device>& Uv) {
    const auto lrm = to_host(L_rm), urm = to_host(U_rm);
    const auto le = to_host(L_ent2), ue = to_host(U_ent2);
    const auto lv = to_host(Lv), uv = to_host(Uv);
    EXPECT((size_t)lrm[n] == nnzL && (size_t)urm[n] == nnzU && lrm[0] == 0 && urm[0] == 0);
    bool graph = true, values = true;
    for (int i = 0; i < n && graph; ++i) {
      size_t p = lrm[i], q = urm[i];
      for (int j = 0; j < i; ++j)
        if (d.in(i, j)) { graph = graph && p < (size_t)lrm[i + 1] && le[p] == j; values = values && graph && close(lv[p], d.at(i, j)); ++p; }
      graph  = graph && p + 1 == (size_t)lrm[i + 1] && le[p] == i;          // the unit diagonal last
      values = values && graph && lv[p] == (scalar)1;
      for (int j = i; j < n; ++j)
        if (d.in(i, j)) { graph = graph && q < (size_t)urm[i + 1] && ue[q] == j; values = values && graph && close(uv[q], d.at(i, j)); ++q; }
      graph = graph && q == (size_t)urm[i + 1];
    }
    EXPECT(graph);
    EXPECT(values);
  };
  check(L_val2, U_val2);

  // the deprecated Experimental:: names forward; a second symbolic call on the handle, numeric twice on one analysis
  KokkosSparse::Experimental::spiluk_symbolic(&kh, fill, A_rm, A_ent, L_rm, L_ent2, U_rm, U_ent2);
  Kokkos::deep_copy(L_val2, std::numeric_limits<scalar>::quiet_NaN());
  Kokkos::deep_copy(U_val2, std::numeric_limits<scalar>::quiet_NaN());
  KokkosSparse::Experimental::spiluk_numeric(&kh, fill, A_rm, A_ent, A_val, L_rm, L_ent2, L_val2, U_rm, U_ent2, U_val2);
  KokkosSparse::spiluk_numeric(&kh, fill, A_rm, A_ent, A_val, L_rm, L_ent2, L_val2, U_rm, U_ent2, U_val2);
  Kokkos::fence();
  check(L_val2, U_val2);

  // one entry too few: the reference's exception text with the true count; the handle is left without an analysis
  if (nnzU > 1) {
    Kokkos::View<int*, device> U_small("U_small", nnzU - 1);
    threw = false;
    try { KokkosSparse::spiluk_symbolic(&kh, fill, A_rm, A_ent, L_rm, L_ent2, U_rm, U_small); }
    catch (const std::runtime_error& e) {
      threw = std::string(e.what()).find("U_entries's extent must be larger than " + std::to_string(nnzU - 1) + ", must be at least " + std::to_string(nnzU)) !=
              std::string::npos;
    }
    EXPECT(threw && !sh->is_symbolic_complete());
  }
  // reset_handle: a fresh analysis state
  sh->reset_handle(n, nnzL, nnzU);
  EXPECT(!sh->is_symbolic_complete() && (size_t)sh->get_nnzL() == nnzL && sh->get_num_levels() == 0);
  KokkosSparse::spiluk_symbolic(&kh, fill, A_rm, A_ent, L_rm, L_ent2, U_rm, U_ent2);
  EXPECT(sh->is_symbolic_complete());
  kh.destroy_spiluk_handle();
  EXPECT(kh.get_spiluk_handle() == nullptr);
}

int main() {
  Kokkos::initialize();
  {
    unsigned seed = 1;
    for (int fill : {0, 2}) {
      run_case<double, int>(7, 6, fill, seed++);
      run_case<float, size_t>(9, 5, fill, seed++);
      run_case<double, size_t>(1, 1, fill, seed++);
    }
    using KH = KokkosKernels::Experimental::KokkosKernelsHandle<int, int, double, Kokkos::HIP, Kokkos::HIPSpace, Kokkos::HIPSpace>;
    KH kh;
    bool threw = false;                                            // the block variant is not supported
    try { kh.create_spiluk_handle(SPILUKAlgorithm::SEQLVLSCHD_TP1, 4, 8, 8, 2); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("not supported") != std::string::npos; }
    EXPECT(threw && kh.get_spiluk_handle() == nullptr);
    Kokkos::View<int*, device> rm("rm", 5), ent("ent", 4);
    threw = false;                                                 // no SPILUK sub-handle: std::invalid_argument
    try { KokkosSparse::spiluk_symbolic(&kh, 0, rm, ent, rm, ent, rm, ent); } catch (const std::invalid_argument&) { threw = true; }
    EXPECT(threw);
  }
  Kokkos::finalize();
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("spiluk drop-in: all passed\n");
  return 0;
}
