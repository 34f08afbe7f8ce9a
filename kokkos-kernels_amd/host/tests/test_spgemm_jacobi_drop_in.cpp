// Host-side test of the spgemm_jacobi drop-in header (run on the GPU by tests/test_gpu_spgemm_jacobi_host_api.py):
// KokkosSparse::Experimental::spgemm_jacobi after KokkosSparse::spgemm_symbolic, for double / int and float / size_t, on the 7-point
// lattice 6 x 5 x 4 squared.  The values are small signed integers times 2^-4, omega = 0.5 and dinv_i = +-2^e / omega, so every partial sum
// of C = B - omega D^-1 (A B) is representable in float in any order: structure and values are compared with `==` against the definition
// summed here in long double.  dinv is a rank-2 view with one column (the reference's) in one case and a rank-1 view in the other.  Also:
// the reference's exception and its text for a transposed operand, a call before the symbolic phase, a row of A without its diagonal.
#include <cstdio>
#include <map>
#include <string>
#include <vector>
#include "KokkosSparse_spgemm.hpp"
#include "KokkosSparse_spgemm_jacobi.hpp"

using device = Kokkos::Device<Kokkos::HIP, Kokkos::HIPSpace>;
static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

template <class size_type, class scalar> struct Host { int n = 0; std::vector<size_type> rm; std::vector<int> ent; std::vector<scalar> val; };

static unsigned next_random(unsigned& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

template <class size_type, class scalar> Host<size_type, scalar> make_lattice(int nx, int ny, int nz, unsigned seed, bool diagonal = true) {
  Host<size_type, scalar> A;
  A.n = nx * ny * nz;
  A.rm.assign(A.n + 1, 0);
  const int d[7][3] = {{0, 0, -1}, {0, -1, 0}, {-1, 0, 0}, {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};      // ascending columns
  for (int i = 0; i < A.n; ++i) {
    const int x = i % nx, y = (i / nx) % ny, z = i / (nx * ny);
    for (auto& o : d) {
      if (x + o[0] < 0 || x + o[0] >= nx || y + o[1] < 0 || y + o[1] >= ny || z + o[2] < 0 || z + o[2] >= nz) continue;
      if (!diagonal && !o[0] && !o[1] && !o[2]) continue;
      A.ent.push_back(i + o[0] + nx * (o[1] + ny * o[2]));
      const int mag = 1 + (int)(next_random(seed) % 7);
      A.val.push_back((scalar)((next_random(seed) & 1) ? -mag : mag) / (scalar)16);
    }
    A.rm[i + 1] = (size_type)A.ent.size();
  }
  return A;
}

template <class V, class T> V to_device(const char* label, const std::vector<T>& h) {
  V v(label, h.size());
  if (!h.empty()) Kokkos::deep_copy(v, typename V::HostMirror(const_cast<T*>(h.data()), h.size()));
  return v;
}
template <class V> std::vector<typename V::non_const_value_type> to_host(const V& v) {
  auto h = Kokkos::create_mirror_view(v);
  Kokkos::deep_copy(h, v);
  return std::vector<typename V::non_const_value_type>(h.data(), h.data() + h.extent(0));
}

template <class size_type, class scalar, bool RANK2> void run_case() {
  using KH        = KokkosKernels::Experimental::KokkosKernelsHandle<size_type, int, scalar, Kokkos::HIP, Kokkos::HIPSpace, Kokkos::HIPSpace>;
  using rowmap_t  = Kokkos::View<size_type*, device>;
  using entries_t = Kokkos::View<int*, device>;
  using values_t  = Kokkos::View<scalar*, device>;
  const auto A = make_lattice<size_type, scalar>(6, 5, 4, 7u);
  const auto B = make_lattice<size_type, scalar>(6, 5, 4, 99u);
  const int n = A.n;
  const scalar omega = (scalar)0.5;
  std::vector<scalar> dinv(n);
  unsigned seed = 5u;
  for (int i = 0; i < n; ++i) dinv[i] = (scalar)((next_random(seed) & 1) ? -1 : 1) * (scalar)(1 << (next_random(seed) % 3)) / omega;

  // the definition, row by row, in long double
  std::vector<std::map<int, long double>> want(n);
  for (int i = 0; i < n; ++i) {
    for (size_t q = B.rm[i]; q < (size_t)B.rm[i + 1]; ++q) want[i][B.ent[q]] += (long double)B.val[q];
    const long double mult = -(long double)omega * (long double)dinv[i];
    for (size_t p = A.rm[i]; p < (size_t)A.rm[i + 1]; ++p)
      for (size_t q = B.rm[A.ent[p]]; q < (size_t)B.rm[A.ent[p] + 1]; ++q) want[i][B.ent[q]] += (long double)A.val[p] * mult * (long double)B.val[q];
  }

  auto rmA = to_device<rowmap_t>("rmA", A.rm); auto entA = to_device<entries_t>("entA", A.ent); auto valA = to_device<values_t>("valA", A.val);
  auto rmB = to_device<rowmap_t>("rmB", B.rm); auto entB = to_device<entries_t>("entB", B.ent); auto valB = to_device<values_t>("valB", B.val);
  KH kh;
  rowmap_t rmC("rmC", n + 1);
  entries_t entC;
  values_t valC;
  auto call = [&](bool tA, bool tB) {
    if constexpr (RANK2) {
      Kokkos::View<scalar**, Kokkos::LayoutLeft, device> d2("dinv", n, 1);
      Kokkos::deep_copy(d2, typename Kokkos::View<scalar**, Kokkos::LayoutLeft, device>::HostMirror(dinv.data(), n, 1));
      KokkosSparse::Experimental::spgemm_jacobi(&kh, n, n, n, rmA, entA, valA, tA, rmB, entB, valB, tB, rmC, entC, valC, omega, d2);
    } else {
      auto d1 = to_device<values_t>("dinv", dinv);
      KokkosSparse::Experimental::spgemm_jacobi(&kh, n, n, n, rmA, entA, valA, tA, rmB, entB, valB, tB, rmC, entC, valC, omega, d1);
    }
  };
  bool threw = false;
  try { call(false, false); } catch (const std::invalid_argument&) { threw = true; }                 // no SpGEMM sub-handle yet
  EXPECT(threw);
  kh.create_spgemm_handle(KokkosSparse::SPGEMM_KK);
  threw = false;
  try { call(false, false); } catch (const std::invalid_argument&) { threw = true; }                 // before the symbolic phase
  EXPECT(threw);
  KokkosSparse::spgemm_symbolic(&kh, n, n, n, rmA, entA, false, rmB, entB, false, rmC);
  const size_t c_nnz = kh.get_spgemm_handle()->get_c_nnz();
  entC = entries_t("entC", c_nnz);
  valC = values_t("valC", c_nnz);
  for (int t = 1; t < 4; ++t) {
    std::string text;
    try { call(t & 1, t & 2); } catch (const std::runtime_error& e) { text = e.what(); }
    EXPECT(text == "spgemm-jacobi does not support transposed multiply. If you need this case please let kokkos-kernels developers know.\n");
  }
  for (int rep = 0; rep < 2; ++rep) {                                                                // the second call reuses entries(C)
    call(false, false);
    const auto h_rm = to_host(rmC); const auto h_ent = to_host(entC); const auto h_val = to_host(valC);
    size_t total = 0;
    for (int i = 0; i < n; ++i) total += want[i].size();
    EXPECT(total == c_nnz && (size_t)h_rm[n] == c_nnz);
    bool same = total == c_nnz;
    for (int i = 0; same && i < n; ++i) {
      size_t q = h_rm[i];
      same = (size_t)(h_rm[i + 1] - h_rm[i]) == want[i].size();
      for (auto it = want[i].begin(); same && it != want[i].end(); ++it, ++q)
        same = h_ent[q] == it->first && (long double)h_val[q] == it->second && (long double)(scalar)it->second == it->second;
    }
    EXPECT(same);
  }
  // a row of A without its diagonal: the row of B is not inside the row of A * B on this lattice's corner
  {
    const auto X = make_lattice<size_type, scalar>(6, 5, 4, 3u, false);
    auto rmX = to_device<rowmap_t>("rmX", X.rm); auto entX = to_device<entries_t>("entX", X.ent); auto valX = to_device<values_t>("valX", X.val);
    std::vector<size_type> irm(n + 1); std::vector<int> ient(n); std::vector<scalar> ival(n, (scalar)1);
    for (int i = 0; i < n; ++i) { irm[i + 1] = (size_type)(i + 1); ient[i] = i; }
    auto rmI = to_device<rowmap_t>("rmI", irm); auto entI = to_device<entries_t>("entI", ient); auto valI = to_device<values_t>("valI", ival);
    KH kx; kx.create_spgemm_handle();
    rowmap_t rmY("rmY", n + 1);
    KokkosSparse::spgemm_symbolic(&kx, n, n, n, rmX, entX, false, rmI, entI, false, rmY);
    entries_t entY("entY", kx.get_spgemm_handle()->get_c_nnz());
    values_t valY("valY", kx.get_spgemm_handle()->get_c_nnz());
    auto d1 = to_device<values_t>("dinv", dinv);
    std::string text;
    try { KokkosSparse::Experimental::spgemm_jacobi(&kx, n, n, n, rmX, entX, valX, false, rmI, entI, valI, false, rmY, entY, valY, omega, d1); }
    catch (const std::runtime_error& e) { text = e.what(); }
    EXPECT(text.find("row 0 of B") != std::string::npos);
  }
}

int main() {
  run_case<int, double, true>();
  run_case<size_t, float, false>();
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("all passed\n");
  return 0;
}
