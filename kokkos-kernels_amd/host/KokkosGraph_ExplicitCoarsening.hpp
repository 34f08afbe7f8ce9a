// KokkosGraph::Experimental::graph_explicit_coarsen / graph_explicit_coarsen_with_inverse_map with the reference's names and argument
// order (graph/src/KokkosGraph_ExplicitCoarsening.hpp:35-92), over the C ABI (kkamd_graph_explicit_coarsen).  compress = true gives the
// reference's result exactly.  compress = false: the reference's rows depend on atomics and a 512-slot hash table; here a row holds the
// cluster's vertices in ascending order, their entries in stored order, every cross-cluster entry kept (the same set per row).  The
// inverse map lists the vertices of a cluster in ascending order (the reference leaves that order to an atomic).
#pragma once
#include <type_traits>
#include <utility>
#include "Kokkos_Shim.hpp"
#include "kkamd_status.hpp"

namespace KokkosGraph {
namespace Experimental {

namespace Impl {
template <class fine_rowmap_t, class fine_entries_t, class labels_t, class coarse_rowmap_t, class coarse_entries_t, class ordinal_view_t>
void explicit_coarsen(const fine_rowmap_t& fineRowmap, const fine_entries_t& fineEntries, const labels_t& labels, int64_t numCoarseVerts,
                      coarse_rowmap_t& coarseRowmap, coarse_entries_t& coarseEntries, ordinal_view_t* inverseOffsets, ordinal_view_t* inverseLabels,
                      bool compress) {
  using size_type = typename fine_rowmap_t::non_const_value_type;
  using lno_t     = typename fine_entries_t::non_const_value_type;
  static_assert(std::is_same<lno_t, typename coarse_entries_t::non_const_value_type>::value,
                "graph_explicit_coarsen: The coarse and fine entry Views have different value types.");
  static_assert(std::is_same<size_type, typename coarse_rowmap_t::non_const_value_type>::value,
                "graph_explicit_coarsen (kkamd): the coarse row map has the fine offset type");
  static_assert(sizeof(lno_t) == 4, "graph_explicit_coarsen (kkamd): ordinals are 32-bit");
  using KokkosSparse::Impl::kkamd_check;
  constexpr int ot = KokkosSparse::Impl::kkamd_offset<size_type>::value;
  const int64_t n = fineRowmap.extent(0) ? (int64_t)fineRowmap.extent(0) - 1 : 0;
  coarse_rowmap_t rm("CoarseRowmap", (size_t)numCoarseVerts + 1);
  ordinal_view_t inv_off, inv_lab;
  if (inverseOffsets) {
    inv_off = ordinal_view_t("ClusterOffsets", (size_t)numCoarseVerts + 1);
    inv_lab = ordinal_view_t(Kokkos::view_alloc(Kokkos::WithoutInitializing, "ClusterVerts"), (size_t)n);
  }
  // one call, with room for the fine graph's entry count: the upper bound of the coarse graph; the result is copied to its own extent
  int64_t nnz = 0;
  const int64_t room_items = (int64_t)fineEntries.extent(0);
  coarse_entries_t room(Kokkos::view_alloc(Kokkos::WithoutInitializing, "CoarseEntries room"), (size_t)room_items);
  kkamd_check(kkamd_graph_explicit_coarsen(n, fineRowmap.data(), ot, (const int32_t*)fineEntries.data(), (const int32_t*)labels.data(), numCoarseVerts,
                                           compress ? 1 : 0, (void*)rm.data(), (int32_t*)room.data(), room_items, &nnz, (int32_t*)inv_off.data(),
                                           (int32_t*)inv_lab.data(), nullptr));
  coarse_entries_t ent(Kokkos::view_alloc(Kokkos::WithoutInitializing, "CoarseEntries"), (size_t)nnz);
  Kokkos::deep_copy(ent, Kokkos::subview(room, std::make_pair(0, (int)nnz)));
  coarseRowmap  = rm;
  coarseEntries = ent;
  if (inverseOffsets) { *inverseOffsets = inv_off; *inverseLabels = inv_lab; }
}
}  // namespace Impl

// Given a CRS graph and coarse labels, produce a new CRS graph representing the coarsened graph.  If A is nonsquare, entries in
// columns >= numVerts are discarded.  The labels should be in the range [0, numCoarseVerts).  If compress, sort and merge entries in
// each row.
template <typename device_t, typename fine_rowmap_t, typename fine_entries_t, typename labels_t, typename coarse_rowmap_t, typename coarse_entries_t>
void graph_explicit_coarsen(const fine_rowmap_t& fineRowmap, const fine_entries_t& fineEntries, const labels_t& labels,
                            typename fine_entries_t::non_const_value_type numCoarseVerts, coarse_rowmap_t& coarseRowmap,
                            coarse_entries_t& coarseEntries, bool compress = true) {
  Impl::explicit_coarsen<fine_rowmap_t, fine_entries_t, labels_t, coarse_rowmap_t, coarse_entries_t, coarse_entries_t>(
      fineRowmap, fineEntries, labels, numCoarseVerts, coarseRowmap, coarseEntries, nullptr, nullptr, compress);
}

// Same as above, but also produce the map from coarse vertices to fine vertices (inverse map of labels)
template <typename device_t, typename fine_rowmap_t, typename fine_entries_t, typename labels_t, typename coarse_rowmap_t, typename coarse_entries_t,
          typename ordinal_view_t>
void graph_explicit_coarsen_with_inverse_map(const fine_rowmap_t& fineRowmap, const fine_entries_t& fineEntries, const labels_t& labels,
                                             typename fine_entries_t::non_const_value_type numCoarseVerts, coarse_rowmap_t& coarseRowmap,
                                             coarse_entries_t& coarseEntries, ordinal_view_t& inverseOffsets, ordinal_view_t& inverseLabels,
                                             bool compress = true) {
  Impl::explicit_coarsen(fineRowmap, fineEntries, labels, numCoarseVerts, coarseRowmap, coarseEntries, &inverseOffsets, &inverseLabels, compress);
}

}  // namespace Experimental
}  // namespace KokkosGraph
