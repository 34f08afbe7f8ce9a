// Host-side test of the ParILUT drop-in headers (run on the GPU by tests/test_gpu_par_ilut_host_api.py):
// KokkosSparse::Experimental::par_ilut_symbolic / par_ilut_numeric through KokkosKernelsHandle::create_par_ilut_handle for (double, int
// offsets) and (float, size_t offsets) on the reference's 4 x 4 fixture (nnzL 10, nnzU 8, the expected factors to 2 decimals, the six views
// resized to the factors' sizes), the handle's defaults, setters and results, numeric before symbolic, a matrix that is not sorted, the
// matrix without rows; then par_ilut, LUPrec and gmres on a diagonally dominant banded matrix built here: fewer iterations than without the
// preconditioner, the true residual, recomputed here in double from the solution, under the tolerance in double (1e-8) and under twice the
// tolerance in float (1e-5: the solver's own residual is a float one).
#include <cmath>
#include <cstdio>
#include <vector>
#include "KokkosSparse_par_ilut.hpp"
#include "KokkosSparse_gmres.hpp"
#include "KokkosSparse_LUPrec.hpp"

using device = Kokkos::Device<Kokkos::HIP, Kokkos::HIPSpace>;
static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

template <class T> Kokkos::View<T*, device> to_device(const std::vector<T>& h, const char* label) {
  Kokkos::View<T*, device> d(label, h.size());
  auto m = Kokkos::create_mirror_view(d);
  for (size_t i = 0; i < h.size(); ++i) m(i) = h[i];
  Kokkos::deep_copy(d, m);
  return d;
}
template <class V> std::vector<typename V::non_const_value_type> to_host(const V& d) {
  auto m = Kokkos::create_mirror_view(d);
  Kokkos::deep_copy(m, d);
  std::vector<typename V::non_const_value_type> h(d.extent(0));
  for (size_t i = 0; i < h.size(); ++i) h[i] = m(i);
  return h;
}

template <class scalar, class size_type> struct Host {
  int n = 0;
  std::vector<size_type> rm{0};
  std::vector<int> ent;
  std::vector<scalar> val;
  void add_row(const std::vector<std::pair<int, double>>& row) {
    for (auto& e : row) { ent.push_back(e.first); val.push_back((scalar)e.second); }
    rm.push_back((size_type)ent.size());
    ++n;
  }
};

// five off-diagonals within +-8 of the row from a small generator, the diagonal 1.5 times 1 + sum |off-diagonals|
template <class scalar, class size_type> Host<scalar, size_type> banded(int n) {
  Host<scalar, size_type> A;
  unsigned s = 12345u;
  auto next = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  for (int i = 0; i < n; ++i) {
    std::vector<double> v(17, 0.0);
    for (int k = 0; k < 5; ++k) {
      const int c = i - 8 + (int)(next() % 17u);
      if (c < 0 || c >= n || c == i) continue;
      v[c - i + 8] = ((double)(next() % 2001u) - 1000.0) / 1000.0;
    }
    double sum = 1.0;
    for (double x : v) sum += std::fabs(x);
    v[8] = 1.5 * sum;
    std::vector<std::pair<int, double>> row;
    for (int k = 0; k < 17; ++k) if (v[k] != 0.0) row.push_back({i - 8 + k, v[k]});
    A.add_row(row);
  }
  return A;
}

template <class scalar, class size_type> void run(const char* label) {
  using KH  = KokkosKernels::Experimental::KokkosKernelsHandle<size_type, int, scalar, Kokkos::HIP, Kokkos::HIPSpace, Kokkos::HIPSpace>;
  using crs = KokkosSparse::CrsMatrix<scalar, int, device, void, size_type>;
  using RowMap  = Kokkos::View<size_type*, device>;
  using Entries = Kokkos::View<int*, device>;
  using Values  = Kokkos::View<scalar*, device>;
  using namespace KokkosSparse::Experimental;
  const bool dbl = sizeof(scalar) == 8;
  {  // the reference's fixture
    const double D[4][4] = {{1., 6., 4., 7.}, {2., -5., 0., 8.}, {0.5, -3., 6., 0.}, {0.2, -0.5, -9., 0.}};
    const double eL[4][4] = {{1., 0., 0., 0.}, {2., 1., 0., 0.}, {0.50, 0.35, 1., 0.}, {0., 0., -1.32, 1.}};
    const double eU[4][4] = {{1., 6., 4., 7.}, {0., -17., -8., -6.}, {0., 0., 6.82, 0.}, {0., 0., 0., 0.}};
    Host<scalar, size_type> A;
    for (int i = 0; i < 4; ++i) {
      std::vector<std::pair<int, double>> row;
      for (int c = 0; c < 4; ++c) if (D[i][c] != 0) row.push_back({c, D[i][c]});
      A.add_row(row);
    }
    auto rm = to_device(A.rm, "rm"); auto ent = to_device(A.ent, "ent"); auto val = to_device(A.val, "val");
    KH kh;
    EXPECT(kh.get_par_ilut_handle() == nullptr);
    kh.create_par_ilut_handle();
    auto* ih = kh.get_par_ilut_handle();
    EXPECT(ih->get_max_iter() == 20 && std::fabs((double)ih->get_residual_norm_delta_stop() - 1e-2) < 1e-8 && (double)ih->get_fill_in_limit() == 0.75);
    EXPECT(!ih->get_async_update() && !ih->get_verbose() && ih->get_num_iters() == -1 && (double)ih->get_end_rel_res() == -1.0);
    ih->set_async_update(false);
    RowMap L_rm("L_rm", 5), U_rm("U_rm", 5);
    Entries L_ent("L_ent", 1), U_ent("U_ent", 1);
    Values L_val("L_val", 1), U_val("U_val", 1);
    bool threw = false;
    try { par_ilut_numeric(&kh, rm, ent, val, L_rm, L_ent, L_val, U_rm, U_ent, U_val); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("par_ilut_symbolic must be called before par_ilut_numeric.") != std::string::npos; }
    EXPECT(threw);
    par_ilut_symbolic(&kh, rm, ent, L_rm, U_rm);
    EXPECT(ih->is_symbolic_complete() && ih->get_nnzL() == (size_type)10 && ih->get_nnzU() == (size_type)8 && ih->get_nrows() == (size_type)4);
    Kokkos::resize(L_ent, ih->get_nnzL()); Kokkos::resize(L_val, ih->get_nnzL());
    Kokkos::resize(U_ent, ih->get_nnzU()); Kokkos::resize(U_val, ih->get_nnzU());
    par_ilut_numeric(&kh, rm, ent, val, L_rm, L_ent, L_val, U_rm, U_ent, U_val);
    EXPECT(ih->get_num_iters() == 4 && (double)ih->get_end_rel_res() >= 0);
    auto check = [&](const RowMap& f_rm, const Entries& f_ent, const Values& f_val, const double (*exp)[4]) {
      auto r = to_host(f_rm); auto e = to_host(f_ent); auto v = to_host(f_val);
      EXPECT(e.size() == (size_t)r[4] && v.size() == (size_t)r[4]);            // resized to the factor's size
      double dense[4][4] = {};
      for (int i = 0; i < 4; ++i) for (size_type p = r[i]; p < r[i + 1]; ++p) dense[i][e[p]] = (double)v[p];
      for (int i = 0; i < 4; ++i) for (int c = 0; c < 4; ++c) EXPECT(std::round(dense[i][c] * 100.0) / 100.0 == exp[i][c]);
    };
    check(L_rm, L_ent, L_val, eL);
    check(U_rm, U_ent, U_val, eU);
    // a second numeric call on the same handle gives the same factors
    auto first = to_host(U_val);
    par_ilut_numeric(&kh, rm, ent, val, L_rm, L_ent, L_val, U_rm, U_ent, U_val);
    EXPECT(first == to_host(U_val));
    // a row that is not sorted: reported, with the reference's assertion text
    std::vector<int> bad_ent = A.ent; std::swap(bad_ent[4], bad_ent[5]);
    auto bad = to_device(bad_ent, "bad");
    threw = false;
    try { par_ilut_symbolic(&kh, rm, bad, L_rm, U_rm); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("row 1:") != std::string::npos && std::string(e.what()).find("is your A matrix sorted?") != std::string::npos; }
    EXPECT(threw && !ih->is_symbolic_complete());
    kh.destroy_par_ilut_handle();
    EXPECT(kh.get_par_ilut_handle() == nullptr);
  }
  {  // no rows (the reference's zerorow test): 0 iterations, residual 0
    KH kh;
    kh.create_par_ilut_handle();
    RowMap rm("rm", 0), L_rm("L_rm", 0), U_rm("U_rm", 0);
    Entries ent("ent", 0), L_ent("L_ent", 0), U_ent("U_ent", 0);
    Values val("val", 0), L_val("L_val", 0), U_val("U_val", 0);
    par_ilut_symbolic(&kh, rm, ent, L_rm, U_rm);
    EXPECT(kh.get_par_ilut_handle()->get_nnzL() == 0 && kh.get_par_ilut_handle()->get_nnzU() == 0);
    par_ilut_numeric(&kh, rm, ent, val, L_rm, L_ent, L_val, U_rm, U_ent, U_val);
    EXPECT(kh.get_par_ilut_handle()->get_num_iters() == 0 && (double)kh.get_par_ilut_handle()->get_end_rel_res() == 0.0);
    EXPECT(L_ent.extent(0) == 0 && U_val.extent(0) == 0);
  }
  {  // par_ilut, then LUPrec, then gmres
    const int n = 300;
    auto H = banded<scalar, size_type>(n);
    auto rm = to_device(H.rm, "rm"); auto ent = to_device(H.ent, "ent"); auto val = to_device(H.val, "val");
    crs A("A", n, n, H.ent.size(), val, rm, ent);
    const scalar tol = dbl ? (scalar)1e-8 : (scalar)1e-5;
    KH kh;
    kh.create_gmres_handle(15, tol);
    kh.create_par_ilut_handle();
    auto* gh = kh.get_gmres_handle();
    auto* ih = kh.get_par_ilut_handle();
    RowMap L_rm("L_rm", n + 1), U_rm("U_rm", n + 1);
    par_ilut_symbolic(&kh, rm, ent, L_rm, U_rm);
    Entries L_ent("L_ent", ih->get_nnzL()), U_ent("U_ent", ih->get_nnzU());
    Values L_val("L_val", ih->get_nnzL()), U_val("U_val", ih->get_nnzU());
    par_ilut_numeric(&kh, rm, ent, val, L_rm, L_ent, L_val, U_rm, U_ent, U_val);
    EXPECT(ih->get_num_iters() >= 1 && ih->get_num_iters() <= 20);
    crs L("L", n, n, L_val.extent(0), L_val, L_rm, L_ent), U("U", n, n, U_val.extent(0), U_val, U_rm, U_ent);
    auto solve = [&](Preconditioner<crs>* P) {
      Values B("b", n), X("x", n);
      Kokkos::deep_copy(B, (scalar)1);
      gmres(&kh, A, B, X, P);
      auto x = to_host(X);
      double r2 = 0;
      for (int i = 0; i < n; ++i) {
        double s = 1.0;
        for (size_type p = H.rm[i]; p < H.rm[i + 1]; ++p) s -= (double)H.val[p] * (double)x[H.ent[p]];
        r2 += s * s;
      }
      return std::sqrt(r2 / n);
    };
    using GH = typename KH::GMRESHandleType;
    const double res_plain = solve(nullptr);
    const int plain = gh->get_num_iters();
    EXPECT(plain > 0 && gh->get_conv_flag_val() == GH::Conv && res_plain < (dbl ? 1.0 : 2.0) * (double)tol);
    gh->reset_handle(15, tol);
    LUPrec<crs, KH> P(L, U);
    const double res_pre = solve(&P);
    const int pre = gh->get_num_iters();
    EXPECT(gh->get_conv_flag_val() == GH::Conv && res_pre < (dbl ? 1.0 : 2.0) * (double)tol);
    EXPECT(pre < plain);
    std::printf("%s: gmres iterations %d plain, %d with par_ilut + LUPrec (par_ilut iterations %d)\n", label, plain, pre, ih->get_num_iters());
  }
  std::printf("%s done\n", label);
}

int main() {
  Kokkos::initialize();
  run<double, int>("double / int offsets");
  run<float, size_t>("float / size_t offsets");
  Kokkos::finalize();
  if (failures) { std::printf("%d FAILED\n", failures); return 1; }
  std::printf("all passed\n");
  return 0;
}
