// Host-side test of the GMRES drop-in headers (run on the GPU by tests/test_gpu_gmres_host_api.py): KokkosSparse::Experimental::gmres
// through KokkosKernelsHandle::create_gmres_handle for (double, int offsets) and (float, size_t offsets), CGS2 and MGS; MatrixPrec
// (Jacobi) and LUPrec (the exact factors of a tridiagonal matrix: one iteration); a user's subclass of Preconditioner whose virtual apply
// is reached through the callback kind; the handle's setters, reset_handle and results; the dimension check's text and m <= 0.
// The matrices are built here: the tridiagonal (4, -1) of n = 513 and the 5-point stencil of the tests (4, -1.5, -0.5, -1.25, -0.75 on
// 12 x 11), b = 1.  Checked: the true residual recomputed in double on the host, and the iteration counts of the Python restatement
// (13 and 6 for the tridiagonal, 1 with its factors, 38 for the stencil in double).
#include <cmath>
#include <cstdio>
#include <vector>
#include "KokkosSparse_gmres.hpp"
#include "KokkosSparse_MatrixPrec.hpp"
#include "KokkosSparse_LUPrec.hpp"

using device = Kokkos::Device<Kokkos::HIP, Kokkos::HIPSpace>;
static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

template <class scalar, class size_type> struct Host {
  int n = 0;
  std::vector<size_type> rm;
  std::vector<int> ent;
  std::vector<scalar> val;
  Host() { rm.push_back(0); }
  void add_row(const std::vector<std::pair<int, double>>& row) {
    for (auto& e : row) { ent.push_back(e.first); val.push_back((scalar)e.second); }
    rm.push_back((size_type)ent.size());
    ++n;
  }
};

template <class scalar, class size_type> using Crs = KokkosSparse::CrsMatrix<scalar, int, device, void, size_type>;

template <class scalar, class size_type> Crs<scalar, size_type> upload(const Host<scalar, size_type>& H) {
  using crs = Crs<scalar, size_type>;
  typename crs::row_map_type::non_const_type rm("rm", H.rm.size());
  typename crs::index_type::non_const_type ent("ent", H.ent.size());
  typename crs::values_type::non_const_type val("val", H.val.size());
  auto rm_h = Kokkos::create_mirror_view(rm); auto ent_h = Kokkos::create_mirror_view(ent); auto val_h = Kokkos::create_mirror_view(val);
  for (size_t i = 0; i < H.rm.size(); ++i) rm_h(i) = H.rm[i];
  for (size_t i = 0; i < H.ent.size(); ++i) { ent_h(i) = H.ent[i]; val_h(i) = H.val[i]; }
  Kokkos::deep_copy(rm, rm_h); Kokkos::deep_copy(ent, ent_h); Kokkos::deep_copy(val, val_h);
  return crs("A", H.n, H.n, H.ent.size(), val, rm, ent);
}

template <class scalar, class size_type> Host<scalar, size_type> tridiagonal(int n) {
  Host<scalar, size_type> A;
  for (int i = 0; i < n; ++i) {
    std::vector<std::pair<int, double>> row;
    if (i > 0) row.push_back({i - 1, -1.0});
    row.push_back({i, 4.0});
    if (i < n - 1) row.push_back({i + 1, -1.0});
    A.add_row(row);
  }
  return A;
}

template <class scalar, class size_type> Host<scalar, size_type> conv2d(int nx, int ny) {
  Host<scalar, size_type> A;
  for (int y = 0; y < ny; ++y) for (int x = 0; x < nx; ++x) {
    const int i = y * nx + x;
    std::vector<std::pair<int, double>> row;
    if (y > 0) row.push_back({i - nx, -1.25});
    if (x > 0) row.push_back({i - 1, -1.5});
    row.push_back({i, 4.0});
    if (x < nx - 1) row.push_back({i + 1, -0.5});
    if (y < ny - 1) row.push_back({i + nx, -0.75});
    A.add_row(row);
  }
  return A;
}

template <class scalar, class size_type> double true_rel_res(const Host<scalar, size_type>& A, const std::vector<scalar>& x) {
  double r2 = 0, b2 = 0;
  for (int i = 0; i < A.n; ++i) {
    double s = 1.0;
    for (size_type p = A.rm[i]; p < A.rm[i + 1]; ++p) s -= (double)A.val[p] * (double)x[A.ent[p]];
    r2 += s * s; b2 += 1.0;
  }
  return std::sqrt(r2 / b2);
}

// a user's preconditioner written against the interface: Jacobi by an SpMV of its own
template <class CRS> struct UserJacobi : KokkosSparse::Experimental::Preconditioner<CRS> {
  using base   = KokkosSparse::Experimental::Preconditioner<CRS>;
  using scalar = typename base::ScalarType;
  CRS Dinv;
  mutable int calls = 0;
  explicit UserJacobi(const CRS& d) : Dinv(d) {}
  void apply(const Kokkos::View<const scalar*, typename base::DEVICE>& X, const Kokkos::View<scalar*, typename base::DEVICE>& Y, const char transM[] = "N",
             scalar alpha = scalar(1), scalar beta = scalar(0)) const override {
    ++calls;
    KokkosSparse::spmv(transM, alpha, Dinv, X, beta, Y);
  }
};

template <class scalar, class size_type> void run(const char* label) {
  using crs = Crs<scalar, size_type>;
  using KH  = KokkosKernels::Experimental::KokkosKernelsHandle<size_type, int, scalar, Kokkos::HIP, Kokkos::HIPSpace, Kokkos::HIPSpace>;
  using GH  = typename KH::GMRESHandleType;
  const bool dbl   = sizeof(scalar) == 8;
  const scalar tol = dbl ? (scalar)7.36e-9 : (scalar)7.42e-5;       // between two short residuals of the tridiagonal case (tests/gmres_cases.py)
  auto solve = [&](KH& kh, const Host<scalar, size_type>& H, crs& A, KokkosSparse::Experimental::Preconditioner<crs>* P) {
    Kokkos::View<scalar*, device> B("b", H.n), X("x", H.n);
    Kokkos::deep_copy(B, (scalar)1);
    KokkosSparse::Experimental::gmres(&kh, A, B, X, P);
    auto X_h = Kokkos::create_mirror_view(X);
    Kokkos::deep_copy(X_h, X);
    std::vector<scalar> x(H.n);
    for (int i = 0; i < H.n; ++i) x[i] = X_h(i);
    return true_rel_res(H, x);
  };
  KH kh;
  EXPECT(kh.get_gmres_handle() == nullptr);
  kh.create_gmres_handle(50, tol);
  GH* gh = kh.get_gmres_handle();
  EXPECT(gh->get_m() == 50 && gh->get_max_restart() == 50 && gh->get_ortho() == GH::CGS2 && !gh->get_verbose());
  EXPECT(gh->get_conv_flag_val() == GH::NotRun);

  auto Ht = tridiagonal<scalar, size_type>(513);
  crs At  = upload(Ht);
  for (auto ortho : {GH::CGS2, GH::MGS}) {
    gh->set_ortho(ortho);
    const double res = solve(kh, Ht, At, nullptr);
    EXPECT(gh->get_conv_flag_val() == GH::Conv);
    EXPECT(gh->get_num_iters() == (dbl ? 13 : 6));
    EXPECT(res < 2 * (double)tol && (double)gh->get_end_rel_res() < (double)tol);
  }
  gh->set_ortho(GH::CGS2);
  {  // the exact factors of the tridiagonal matrix: L unit lower bidiagonal, U upper bidiagonal
    Host<scalar, size_type> L, U;
    double u = 4.0;
    for (int i = 0; i < Ht.n; ++i) {
      std::vector<std::pair<int, double>> lrow, urow;
      if (i > 0) { const double l = -1.0 / u; lrow.push_back({i - 1, l}); u = 4.0 + l; }
      lrow.push_back({i, 1.0});
      urow.push_back({i, u});
      if (i < Ht.n - 1) urow.push_back({i + 1, -1.0});
      L.add_row(lrow); U.add_row(urow);
    }
    crs Ld = upload(L), Ud = upload(U);
    KokkosSparse::Experimental::LUPrec<crs, KH> P(Ld, Ud);
    const double res = solve(kh, Ht, At, &P);
    EXPECT(gh->get_conv_flag_val() == GH::Conv && gh->get_num_iters() == 1);
    EXPECT(res < 2 * (double)tol);
  }
  auto Hc = conv2d<scalar, size_type>(12, 11);
  crs Ac  = upload(Hc);
  gh->set_tol(dbl ? (scalar)1e-8 : (scalar)2.23e-5);
  const double res0 = solve(kh, Hc, Ac, nullptr);
  const int plain   = gh->get_num_iters();
  EXPECT(gh->get_conv_flag_val() == GH::Conv && res0 < 2 * (double)gh->get_tol());
  if (dbl) EXPECT(plain == 38);
  {  // Jacobi as MatrixPrec and as a user's subclass
    Host<scalar, size_type> D;
    for (int i = 0; i < Hc.n; ++i) D.add_row({{i, 0.25}});
    crs Dd = upload(D);
    KokkosSparse::Experimental::MatrixPrec<crs> P(Dd);
    const double res1 = solve(kh, Hc, Ac, &P);
    const int with_matrix = gh->get_num_iters();
    EXPECT(gh->get_conv_flag_val() == GH::Conv && std::abs(with_matrix - plain) <= 1 && res1 < 2 * (double)gh->get_tol());
    UserJacobi<crs> Q(Dd);
    const double res2 = solve(kh, Hc, Ac, &Q);
    EXPECT(gh->get_conv_flag_val() == GH::Conv && gh->get_num_iters() == with_matrix && res2 < 2 * (double)gh->get_tol());
    EXPECT(Q.calls == with_matrix + 1);                    // once per iteration and once for the solution update
  }
  // restarts
  gh->set_m(4);
  solve(kh, Hc, Ac, nullptr);
  EXPECT(gh->get_conv_flag_val() == GH::Conv && gh->get("cycles") > 1 && gh->get_num_iters() > 4);
  // errors
  {
    Kokkos::View<scalar*, device> B("b", Hc.n), X("x", Hc.n + 1);
    bool threw = false;
    try { KokkosSparse::Experimental::gmres(&kh, Ac, B, X); }
    catch (const std::runtime_error& e) { threw = std::string(e.what()).find("KokkosSparse::gmres: Dimensions do not match: , A: 132 x 132, x: 133, b: 132") != std::string::npos; }
    EXPECT(threw);
    threw = false;
    try { KH bad; bad.create_gmres_handle(0); }
    catch (const std::invalid_argument& e) { threw = std::string(e.what()).find("gmres: Please choose restart size m greater than zero.") != std::string::npos; }
    EXPECT(threw);
  }
  gh->reset_handle();
  EXPECT(gh->get_m() == 50 && gh->get_conv_flag_val() == GH::NotRun);
  kh.destroy_gmres_handle();
  EXPECT(kh.get_gmres_handle() == nullptr);
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
