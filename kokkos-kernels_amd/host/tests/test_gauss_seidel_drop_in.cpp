// Host-side test of the multicolor Gauss-Seidel drop-in headers (run on the GPU by tests/test_gpu_gauss_seidel_host_api.py):
// KokkosSparse::gauss_seidel_symbolic / gauss_seidel_numeric and the three apply functions through
// KokkosKernelsHandle::create_gs_handle, with and without an execution space instance, under the KokkosSparse::Experimental:: names
// too, for (double, int offsets) and (float, size_t offsets); a rank-2 LayoutLeft view; the given_inverse_diagonal overload;
// get_point_gs_handle()->set_long_row_threshold; destroy_gs_handle.
// The matrix is built here: the 27-point lattice with entries in shuffled order, off-diagonals uniform in (-1, 1) and a dominant
// diagonal.  The expected x is a sequential sweep computed in this program in double, colour by colour with the handle's own colours
// (the rows of one colour do not read one another), compared to a tolerance of a few hundred roundings of the working type.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>
#include "KokkosSparse_gauss_seidel.hpp"

using device = Kokkos::Device<Kokkos::HIP, Kokkos::HIPSpace>;
static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

template <class scalar, class size_type> struct Lattice {
  int n = 0;
  std::vector<size_type> rm;
  std::vector<int> ent;
  std::vector<scalar> val;
};

template <class scalar, class size_type> Lattice<scalar, size_type> make_lattice(int nx, int ny, int nz, unsigned seed) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  Lattice<scalar, size_type> A;
  A.n = nx * ny * nz;
  A.rm.assign(A.n + 1, 0);
  for (int i = 0; i < A.n; ++i) {
    const int x = i % nx, y = (i / nx) % ny, z = i / (nx * ny);
    std::vector<std::pair<int, scalar>> row;
    double sum = 0;
    for (int dz = -1; dz <= 1; ++dz) for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) {
      if ((!dx && !dy && !dz) || x + dx < 0 || x + dx >= nx || y + dy < 0 || y + dy >= ny || z + dz < 0 || z + dz >= nz) continue;
      const scalar a = (scalar)u(g);
      row.push_back({i + dx + nx * (dy + ny * dz), a});
      sum += std::fabs((double)a);
    }
    row.push_back({i, (scalar)((1.0 + sum) * (1.0 + 0.5 * (u(g) + 1.0)) * ((g() & 1) ? 1 : -1))});
    std::shuffle(row.begin(), row.end(), g);
    for (auto& e : row) { A.ent.push_back(e.first); A.val.push_back(e.second); }
    A.rm[i + 1] = (size_type)A.ent.size();
  }
  return A;
}

// one sweep over the colour sets (xadj, adj) in double: sum = y_i - sum_j a_ij x_j over the whole row, x_i += omega * sum * inv_diag_i
template <class L, class scalar>
void host_sweep(const L& A, const std::vector<int>& xadj, const std::vector<int>& adj, const std::vector<double>& inv_diag, const std::vector<scalar>& y,
                std::vector<double>& x, double omega, bool backward) {
  const int C = (int)xadj.size() - 1;
  for (int k = 0; k < C; ++k) {
    const int c = backward ? C - 1 - k : k;
    for (int p = xadj[c]; p < xadj[c + 1]; ++p) {
      const int i = adj[p];
      double sum = (double)y[i];
      for (size_t q = A.rm[i]; q < (size_t)A.rm[i + 1]; ++q) sum -= (double)A.val[q] * x[A.ent[q]];
      x[i] += omega * sum * inv_diag[i];
    }
  }
}

template <class scalar, class V> bool close_to(const V& d_x, int col, const std::vector<double>& expect) {
  auto h = Kokkos::create_mirror_view(d_x);
  Kokkos::deep_copy(h, d_x);
  const double tol = 400.0 * (double)std::numeric_limits<scalar>::epsilon();
  for (size_t i = 0; i < expect.size(); ++i) {
    const double got = V::rank() == 2 ? (double)h.data()[i * h.stride(0) + col * h.stride(1)] : (double)h.data()[i];
    if (!(std::fabs(got - expect[i]) <= tol * (1.0 + std::fabs(expect[i])))) return false;
  }
  return true;
}

template <class scalar, class size_type> void run_case(KokkosSparse::GSAlgorithm algo, int long_row_threshold, unsigned seed) {
  using KH = KokkosKernels::Experimental::KokkosKernelsHandle<size_type, int, scalar, Kokkos::HIP, Kokkos::HIPSpace, Kokkos::HIPSpace>;
  const auto A = make_lattice<scalar, size_type>(7, 6, 5, seed);
  const int n = A.n;
  std::mt19937 g(seed + 99);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  std::vector<scalar> h_x0(n), h_y(n);
  for (int i = 0; i < n; ++i) { h_x0[i] = (scalar)u(g); h_y[i] = (scalar)u(g); }
  std::vector<double> inv_diag(n);
  for (int i = 0; i < n; ++i)
    for (size_t q = A.rm[i]; q < (size_t)A.rm[i + 1]; ++q) if (A.ent[q] == i) inv_diag[i] = 1.0 / (double)A.val[q];

  Kokkos::View<size_type*, device> rm("rm", n + 1);
  Kokkos::View<int*, device> ent("ent", A.ent.size());
  Kokkos::View<scalar*, device> val("val", A.val.size()), x("x", n), y("y", n);
  Kokkos::deep_copy(rm, Kokkos::View<const size_type*, Kokkos::HostSpace>(A.rm.data(), A.rm.size()));
  Kokkos::deep_copy(ent, Kokkos::View<const int*, Kokkos::HostSpace>(A.ent.data(), A.ent.size()));
  Kokkos::deep_copy(val, Kokkos::View<const scalar*, Kokkos::HostSpace>(A.val.data(), A.val.size()));
  Kokkos::deep_copy(y, Kokkos::View<const scalar*, Kokkos::HostSpace>(h_y.data(), h_y.size()));
  auto reset_x = [&]() { Kokkos::deep_copy(x, Kokkos::View<const scalar*, Kokkos::HostSpace>(h_x0.data(), h_x0.size())); };
  auto x0 = [&]() { return std::vector<double>(h_x0.begin(), h_x0.end()); };

  KH kh;
  EXPECT(kh.get_gs_handle() == nullptr);
  kh.create_gs_handle(algo);
  auto* gh = kh.get_point_gs_handle();
  EXPECT(gh == kh.get_gs_handle() && gh->get_algorithm_type() == algo && !gh->is_symbolic_called());
  gh->set_long_row_threshold(long_row_threshold);
  EXPECT((int)gh->get_long_row_threshold() == long_row_threshold);
  bool threw = false;                                   // apply before symbolic: std::invalid_argument
  try { KokkosSparse::forward_sweep_gauss_seidel_apply(&kh, n, n, rm, ent, val, x, y, false, true, (scalar)1, 1); } catch (const std::invalid_argument&) { threw = true; }
  EXPECT(threw);

  // without an execution space
  KokkosSparse::gauss_seidel_symbolic(&kh, n, n, rm, ent, true);
  EXPECT(gh->is_symbolic_called() && !gh->is_numeric_called() && gh->get_num_colors() >= 8);
  EXPECT((gh->get_num_long_rows() > 0) == (long_row_threshold > 0 && long_row_threshold < 27));
  const std::vector<int> colors = gh->export_host("colors"), xadj = gh->export_host("color_xadj"), adj = gh->export_host("color_adj");
  bool proper = true;
  for (int i = 0; i < n; ++i)
    for (size_t q = A.rm[i]; q < (size_t)A.rm[i + 1]; ++q) if (A.ent[q] != i && colors[A.ent[q]] == colors[i]) proper = false;
  EXPECT(proper && (int)xadj.size() == (int)gh->get_num_colors() + 1 && xadj.back() == n);
  KokkosSparse::gauss_seidel_numeric(&kh, n, n, rm, ent, val, true);
  EXPECT(gh->is_numeric_called());

  for (int dir = 0; dir < 3; ++dir) {                   // forward, backward, symmetric; omega 0.9, two iterations
    reset_x();
    auto expect = x0();
    for (int it = 0; it < 2; ++it) {
      if (dir != 1) host_sweep(A, xadj, adj, inv_diag, h_y, expect, 0.9, false);
      if (dir != 0) host_sweep(A, xadj, adj, inv_diag, h_y, expect, 0.9, true);
    }
    if (dir == 0) KokkosSparse::forward_sweep_gauss_seidel_apply(&kh, n, n, rm, ent, val, x, y, false, true, (scalar)0.9, 2);
    if (dir == 1) KokkosSparse::backward_sweep_gauss_seidel_apply(&kh, n, n, rm, ent, val, x, y, false, true, (scalar)0.9, 2);
    if (dir == 2) KokkosSparse::symmetric_gauss_seidel_apply(&kh, n, n, rm, ent, val, x, y, false, true, (scalar)0.9, 2);
    Kokkos::fence();
    EXPECT(close_to<scalar>(x, 0, expect));
  }

  // init_zero_x_vector over a NaN-filled x
  {
    Kokkos::deep_copy(x, std::numeric_limits<scalar>::quiet_NaN());
    std::vector<double> expect(n, 0.0);
    host_sweep(A, xadj, adj, inv_diag, h_y, expect, 1.0, false);
    KokkosSparse::forward_sweep_gauss_seidel_apply(&kh, n, n, rm, ent, val, x, y, true, true, (scalar)1, 1);
    Kokkos::fence();
    EXPECT(close_to<scalar>(x, 0, expect));
  }

  // a rank-2 LayoutLeft view: column v starts from (v + 1) x0 with right-hand side (v + 1) y, which gives (v + 1) times column 0
  {
    const int nv = 3;
    Kokkos::View<scalar**, Kokkos::LayoutLeft, device> X("X", n, nv), Y("Y", n, nv);
    auto hX = Kokkos::create_mirror_view(X);
    auto hY = Kokkos::create_mirror_view(Y);
    for (int v = 0; v < nv; ++v) for (int i = 0; i < n; ++i) { hX(i, v) = (scalar)(v + 1) * h_x0[i]; hY(i, v) = (scalar)(v + 1) * h_y[i]; }
    Kokkos::deep_copy(X, hX);
    Kokkos::deep_copy(Y, hY);
    auto expect = x0();
    host_sweep(A, xadj, adj, inv_diag, h_y, expect, 1.2, false);
    host_sweep(A, xadj, adj, inv_diag, h_y, expect, 1.2, true);
    KokkosSparse::symmetric_gauss_seidel_apply(&kh, n, n, rm, ent, val, X, Y, false, true, (scalar)1.2, 1);
    Kokkos::fence();
    for (int v = 0; v < nv; ++v) {
      std::vector<double> e(n);
      for (int i = 0; i < n; ++i) e[i] = (v + 1) * expect[i];
      EXPECT(close_to<scalar>(X, v, e));
    }
  }

  // with an execution space instance on its own stream; const views of the matrix; the given_inverse_diagonal overload: half the
  // inverse diagonal is omega = 0.5; the KokkosSparse::Experimental:: names
  hipStream_t stream = nullptr;
  EXPECT(hipStreamCreate(&stream) == hipSuccess);
  {
    Kokkos::HIP space(stream);
    typename Kokkos::View<size_type*, device>::const_type c_rm = rm;
    typename Kokkos::View<int*, device>::const_type c_ent = ent;
    typename Kokkos::View<scalar*, device>::const_type c_val = val, c_y = y;
    std::vector<scalar> h_half(n);
    for (int i = 0; i < n; ++i) h_half[i] = (scalar)(0.5 * inv_diag[i]);
    Kokkos::View<scalar*, device> half("half", n);
    Kokkos::deep_copy(half, Kokkos::View<const scalar*, Kokkos::HostSpace>(h_half.data(), h_half.size()));
    typename Kokkos::View<scalar*, device>::const_type c_half = half;
    KokkosSparse::gauss_seidel_symbolic(space, &kh, n, n, c_rm, c_ent, true);
    EXPECT(gh->export_host("colors") == colors && !gh->is_numeric_called());
    KokkosSparse::gauss_seidel_numeric(space, &kh, n, n, c_rm, c_ent, c_val, c_half, true);
    reset_x();
    auto expect = x0();
    host_sweep(A, xadj, adj, inv_diag, h_y, expect, 0.5, true);
    KokkosSparse::backward_sweep_gauss_seidel_apply(space, &kh, n, n, c_rm, c_ent, c_val, x, c_y, false, true, (scalar)1, 1);
    space.fence();
    EXPECT(close_to<scalar>(x, 0, expect));
    KokkosSparse::Experimental::gauss_seidel_numeric(space, &kh, n, n, c_rm, c_ent, c_val, true);   // the computed inverse diagonal again
    reset_x();
    expect = x0();
    host_sweep(A, xadj, adj, inv_diag, h_y, expect, 1.0, false);
    KokkosSparse::Experimental::forward_sweep_gauss_seidel_apply(space, &kh, n, n, c_rm, c_ent, c_val, x, c_y, false, true, (scalar)1, 1);
    space.fence();
    EXPECT(close_to<scalar>(x, 0, expect));
  }
  EXPECT(hipStreamDestroy(stream) == hipSuccess);
  KokkosSparse::Experimental::gauss_seidel_symbolic(&kh, n, n, rm, ent);
  reset_x();
  {
    auto expect = x0();                                 // no numeric call: apply runs it
    host_sweep(A, xadj, adj, inv_diag, h_y, expect, 1.0, false);
    host_sweep(A, xadj, adj, inv_diag, h_y, expect, 1.0, true);
    KokkosSparse::Experimental::symmetric_gauss_seidel_apply(&kh, n, n, rm, ent, val, x, y, false, true, (scalar)1, 1);
    Kokkos::fence();
    EXPECT(close_to<scalar>(x, 0, expect) && gh->is_numeric_called());
  }
  kh.destroy_gs_handle();
  EXPECT(kh.get_gs_handle() == nullptr && kh.get_point_gs_handle() == nullptr);
}

int main() {
  Kokkos::initialize();
  {
    run_case<double, int>(KokkosSparse::GS_DEFAULT, 0, 1);
    run_case<float, size_t>(KokkosSparse::GS_TEAM, 20, 2);
    run_case<double, size_t>(KokkosSparse::GS_PERMUTED, 20, 3);
    run_case<float, int>(KokkosSparse::GS_DEFAULT, 0, 4);
    using KH = KokkosKernels::Experimental::KokkosKernelsHandle<int, int, double, Kokkos::HIP, Kokkos::HIPSpace, Kokkos::HIPSpace>;
    KH kh;
    for (KokkosSparse::GSAlgorithm a : {KokkosSparse::GS_CLUSTER, KokkosSparse::GS_TWOSTAGE}) {
      bool threw = false;
      try { kh.create_gs_handle(a); } catch (const std::runtime_error&) { threw = true; }
      EXPECT(threw && kh.get_gs_handle() == nullptr);
    }
    Kokkos::View<int*, device> rm("rm", 5), ent("ent", 4);
    bool threw = false;                                            // no Gauss-Seidel sub-handle: std::invalid_argument
    try { KokkosSparse::gauss_seidel_symbolic(&kh, 4, 4, rm, ent); } catch (const std::invalid_argument&) { threw = true; }
    EXPECT(threw);
  }
  Kokkos::finalize();
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("gauss-seidel drop-in: all passed\n");
  return 0;
}
