// Host-side test of the MIS-2 / coarsening drop-in headers (run on the GPU by tests/test_gpu_mis2_host_api.py):
// KokkosGraph::graph_d2_mis for both algorithms, graph_mis2_coarsen, graph_mis2_aggregate, mis2_algorithm_name, the deprecated
// KokkosGraph::Experimental:: names, graph_explicit_coarsen and graph_explicit_coarsen_with_inverse_map, for int and size_t offsets.
// The graph is built here: the 7-point lattice 9 x 8 x 7 without its diagonal.  Checked in this program, from the definitions: the set is
// ascending, independent and maximal at distance 2; the labels cover [0, numAggregates), no aggregate is empty and aggregate a holds the
// a-th root; the coarse graph equals the set of cross-aggregate label pairs, sorted; the inverse map lists every cluster ascending.
#include <algorithm>
#include <cstdio>
#include <set>
#include <string>
#include <vector>
#include "KokkosGraph_MIS2.hpp"
#include "KokkosGraph_ExplicitCoarsening.hpp"

using device = Kokkos::Device<Kokkos::HIP, Kokkos::HIPSpace>;
static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

template <class size_type> struct Lattice { int n = 0; std::vector<size_type> rm; std::vector<int> ent; };

template <class size_type> Lattice<size_type> make_lattice(int nx, int ny, int nz) {
  Lattice<size_type> A;
  A.n = nx * ny * nz;
  A.rm.assign(A.n + 1, 0);
  const int d[6][3] = {{-1, 0, 0}, {1, 0, 0}, {0, -1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}};
  for (int i = 0; i < A.n; ++i) {
    const int x = i % nx, y = (i / nx) % ny, z = i / (nx * ny);
    for (auto& o : d) {
      if (x + o[0] < 0 || x + o[0] >= nx || y + o[1] < 0 || y + o[1] >= ny || z + o[2] < 0 || z + o[2] >= nz) continue;
      A.ent.push_back(i + o[0] + nx * (o[1] + ny * o[2]));
    }
    A.rm[i + 1] = (size_type)A.ent.size();
  }
  return A;
}

template <class V> std::vector<typename V::non_const_value_type> to_host(const V& v) {
  auto h = Kokkos::create_mirror_view(v);
  Kokkos::deep_copy(h, v);
  return std::vector<typename V::non_const_value_type>(h.data(), h.data() + h.extent(0));
}

template <class L> void check_set(const L& A, const std::vector<int>& set) {
  std::vector<int> cover(A.n, 0);
  EXPECT(!set.empty() && std::is_sorted(set.begin(), set.end()) && std::adjacent_find(set.begin(), set.end()) == set.end());
  for (int r : set) {
    cover[r] += 1;
    for (size_t q = A.rm[r]; q < (size_t)A.rm[r + 1]; ++q) cover[A.ent[q]] += 1;
  }
  bool independent = true, maximal = true;
  for (int i = 0; i < A.n; ++i) {
    if (cover[i] > 1) independent = false;                   // two members within distance 2 share a closed neighbourhood
    bool reached = cover[i] > 0;
    for (size_t q = A.rm[i]; q < (size_t)A.rm[i + 1]; ++q) reached = reached || cover[A.ent[q]] > 0;
    if (!reached) maximal = false;
  }
  EXPECT(independent);
  EXPECT(maximal);
}

template <class size_type> void run_case() {
  using rowmap_t  = Kokkos::View<size_type*, device>;
  using entries_t = Kokkos::View<int*, device>;
  const auto A = make_lattice<size_type>(9, 8, 7);
  rowmap_t rm("rm", A.rm.size());
  entries_t ent("ent", A.ent.size());
  Kokkos::deep_copy(rm, typename rowmap_t::HostMirror(const_cast<size_type*>(A.rm.data()), A.rm.size()));
  Kokkos::deep_copy(ent, typename entries_t::HostMirror(const_cast<int*>(A.ent.data()), A.ent.size()));
  typename rowmap_t::const_type crm = rm;
  typename entries_t::const_type cent = ent;

  const auto fast    = to_host(KokkosGraph::graph_d2_mis<device>(crm, cent));
  const auto quality = to_host(KokkosGraph::graph_d2_mis<device>(rm, ent, KokkosGraph::MIS2_QUALITY));
  check_set(A, fast);
  check_set(A, quality);
  EXPECT(to_host(KokkosGraph::graph_d2_mis<device>(rm, ent, KokkosGraph::MIS2_FAST)) == fast);     // a function of the graph alone

  int num_coarse = -1, num_agg = -1;
  const auto coarse = to_host(KokkosGraph::graph_mis2_coarsen<device>(rm, ent, num_coarse));
  auto d_labels     = KokkosGraph::graph_mis2_aggregate<device>(crm, cent, num_agg);
  const auto labels = to_host(d_labels);
  EXPECT(num_coarse == (int)fast.size() && num_agg >= num_coarse);
  for (int pass = 0; pass < 2; ++pass) {
    const auto& l = pass ? labels : coarse;
    const int num = pass ? num_agg : num_coarse;
    std::vector<int> size(num, 0);
    bool in_range = (int)l.size() == A.n;
    for (int v : l) { if (v < 0 || v >= num) in_range = false; else size[v] += 1; }
    EXPECT(in_range);
    EXPECT(std::find(size.begin(), size.end(), 0) == size.end());
    for (size_t a = 0; a < fast.size(); ++a) EXPECT(l[fast[a]] == (int)a);   // aggregate a is the a-th root: roots never move
  }

  // the coarse graph against the set of cross-aggregate pairs
  std::set<std::pair<int, int>> pairs;
  for (int i = 0; i < A.n; ++i)
    for (size_t q = A.rm[i]; q < (size_t)A.rm[i + 1]; ++q)
      if (labels[i] != labels[A.ent[q]]) pairs.insert({labels[i], labels[A.ent[q]]});
  rowmap_t c_rm, u_rm;
  entries_t c_ent, u_ent, inv_off, inv_lab;
  KokkosGraph::Experimental::graph_explicit_coarsen<device>(crm, cent, d_labels, num_agg, c_rm, c_ent);
  const auto h_rm = to_host(c_rm);
  const auto h_ent = to_host(c_ent);
  EXPECT((int)h_rm.size() == num_agg + 1 && h_ent.size() == pairs.size() && (size_t)h_rm.back() == pairs.size());
  {
    auto it = pairs.begin();
    bool same = h_ent.size() == pairs.size();
    for (int c = 0; same && c < num_agg; ++c)
      for (size_t q = h_rm[c]; q < (size_t)h_rm[c + 1]; ++q, ++it) same = same && it->first == c && it->second == h_ent[q];
    EXPECT(same);
  }
  KokkosGraph::Experimental::graph_explicit_coarsen_with_inverse_map<device>(rm, ent, d_labels, num_agg, u_rm, u_ent, inv_off, inv_lab, false);
  const auto hu_rm = to_host(u_rm);
  const auto hu_ent = to_host(u_ent);
  const auto h_off = to_host(inv_off);
  const auto h_lab = to_host(inv_lab);
  EXPECT(hu_ent.size() >= h_ent.size() && hu_ent.size() <= A.ent.size() && (int)h_off.size() == num_agg + 1 && (int)h_lab.size() == A.n);
  bool rows_same = true, inverse_ok = h_off[0] == 0 && h_off[num_agg] == A.n;
  for (int c = 0; c < num_agg; ++c) {
    std::set<int> row(hu_ent.begin() + hu_rm[c], hu_ent.begin() + hu_rm[c + 1]);
    rows_same = rows_same && std::vector<int>(row.begin(), row.end()) == std::vector<int>(h_ent.begin() + h_rm[c], h_ent.begin() + h_rm[c + 1]);
    for (int p = h_off[c]; p < h_off[c + 1]; ++p) inverse_ok = inverse_ok && labels[h_lab[p]] == c && (p == h_off[c] || h_lab[p - 1] < h_lab[p]);
  }
  EXPECT(rows_same);
  EXPECT(inverse_ok);

  // the empty graph, and the names
  rowmap_t none;
  int zero = 7;
  EXPECT(KokkosGraph::graph_d2_mis<device>(none, ent).extent(0) == 0);
  EXPECT(KokkosGraph::graph_mis2_aggregate<device>(none, ent, zero).extent(0) == 0 && zero == 0);
}

int main() {
  run_case<int>();
  run_case<size_t>();
  EXPECT(std::string(KokkosGraph::mis2_algorithm_name(KokkosGraph::MIS2_QUALITY)) == "MIS2_QUALITY");
  EXPECT(std::string(KokkosGraph::mis2_algorithm_name(KokkosGraph::MIS2_FAST)) == "MIS2_FAST");
  EXPECT((int)KokkosGraph::MIS2_QUALITY == KKAMD_MIS2_QUALITY && (int)KokkosGraph::MIS2_FAST == KKAMD_MIS2_FAST);
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wdeprecated-declarations"
  {
    using rowmap_t  = Kokkos::View<int*, device>;
    using entries_t = Kokkos::View<int*, device>;
    const auto A = make_lattice<int>(5, 4, 3);
    rowmap_t rm("rm", A.rm.size());
    entries_t ent("ent", A.ent.size());
    Kokkos::deep_copy(rm, rowmap_t::HostMirror(const_cast<int*>(A.rm.data()), A.rm.size()));
    Kokkos::deep_copy(ent, entries_t::HostMirror(const_cast<int*>(A.ent.data()), A.ent.size()));
    int a = 0, b = 0;
    const auto set = to_host(KokkosGraph::Experimental::graph_d2_mis<device>(rm, ent));
    check_set(A, set);
    EXPECT(KokkosGraph::Experimental::graph_mis2_coarsen<device>(rm, ent, a).extent(0) == (size_t)A.n && a == (int)set.size());
    EXPECT(KokkosGraph::Experimental::graph_mis2_aggregate<device>(rm, ent, b).extent(0) == (size_t)A.n && b >= a);
    EXPECT(std::string(KokkosGraph::Experimental::mis2_algorithm_name(KokkosGraph::MIS2_FAST)) == "MIS2_FAST");
    // a graph that is not symmetric is reported
    std::vector<int> drm = {0, 1, 2, 3}, dent = {1, 2, 0};
    rowmap_t r3("rm", 4);
    entries_t e3("ent", 3);
    Kokkos::deep_copy(r3, rowmap_t::HostMirror(drm.data(), 4));
    Kokkos::deep_copy(e3, entries_t::HostMirror(dent.data(), 3));
    bool thrown = false;
    try { (void)KokkosGraph::graph_d2_mis<device>(r3, e3); } catch (const std::runtime_error& e) { thrown = std::string(e.what()).find("not symmetric") != std::string::npos; }
    EXPECT(thrown);
  }
#pragma GCC diagnostic pop
  if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
  std::printf("all passed\n");
  return 0;
}
