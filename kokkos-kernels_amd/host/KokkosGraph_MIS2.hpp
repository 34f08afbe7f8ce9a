// KokkosGraph::graph_d2_mis / graph_mis2_coarsen / graph_mis2_aggregate / mis2_algorithm_name with the reference's names, template
// parameters and return types (graph/src/KokkosGraph_MIS2.hpp:24-121), over the C ABI (kkamd_graph_d2_mis, kkamd_graph_mis2_aggregate;
// include/kkamd.h states the algorithm bit for bit).  The results are the reference's: functions of the graph alone.  Two differences,
// both in kkamd.h: MIS2_QUALITY on a graph whose degrees are all equal takes the degree score as 0 (the reference divides by zero),
// and a graph that is not symmetric is reported (std::runtime_error, "graph is not symmetric") where the reference would not return.
#pragma once
#include <stdexcept>
#include <utility>
#include "Kokkos_Shim.hpp"
#include "kkamd_status.hpp"

namespace KokkosGraph {

enum MIS2_Algorithm { MIS2_QUALITY, MIS2_FAST };

namespace Impl {
using KokkosSparse::Impl::kkamd_check;
using KokkosSparse::Impl::kkamd_offset;
template <class rowmap_t, class colinds_t, class labels_t>
labels_t mis2_labels(const rowmap_t& rowmap, const colinds_t& colinds, int secondary, typename colinds_t::non_const_value_type& num) {
  static_assert(sizeof(typename colinds_t::non_const_value_type) == 4, "KokkosGraph MIS-2 (kkamd): ordinals are 32-bit");
  const int64_t n = (int64_t)rowmap.extent(0) - 1;
  labels_t labels(Kokkos::view_alloc(Kokkos::WithoutInitializing, "AggregateLabels"), (size_t)n);
  int64_t count = 0;
  kkamd_check(kkamd_graph_mis2_aggregate(n, rowmap.data(), kkamd_offset<typename rowmap_t::non_const_value_type>::value, (const int32_t*)colinds.data(),
                                         secondary, (int32_t*)labels.data(), &count, nullptr, nullptr));
  num = (typename colinds_t::non_const_value_type)count;
  return labels;
}
}  // namespace Impl

// Compute a distance-2 maximal independent set, given a symmetric CRS graph.  Returns the vertices in the set, ascending.
// Column indices >= num_verts are ignored.
template <typename device_t, typename rowmap_t, typename colinds_t, typename lno_view_t = typename colinds_t::non_const_type>
lno_view_t graph_d2_mis(const rowmap_t& rowmap, const colinds_t& colinds, MIS2_Algorithm algo = MIS2_FAST) {
  static_assert(sizeof(typename colinds_t::non_const_value_type) == 4, "KokkosGraph::graph_d2_mis (kkamd): ordinals are 32-bit");
  if (rowmap.extent(0) <= 1) return lno_view_t();             // zero vertices means the MIS is empty
  if (algo != MIS2_QUALITY && algo != MIS2_FAST) throw std::invalid_argument("graph_d2_mis: invalid algorithm");
  const int64_t n = (int64_t)rowmap.extent(0) - 1;
  lno_view_t room(Kokkos::view_alloc(Kokkos::WithoutInitializing, "D2MIS room"), (size_t)n);
  int64_t count = 0;
  Impl::kkamd_check(kkamd_graph_d2_mis(n, rowmap.data(), Impl::kkamd_offset<typename rowmap_t::non_const_value_type>::value, (const int32_t*)colinds.data(),
                                       (int)algo, (int32_t*)room.data(), &count, nullptr, nullptr));
  lno_view_t set(Kokkos::view_alloc(Kokkos::WithoutInitializing, "D2MIS"), (size_t)count);
  Kokkos::deep_copy(set, Kokkos::subview(room, std::make_pair(0, (int)count)));
  return set;
}

template <typename device_t, typename rowmap_t, typename colinds_t, typename labels_t = typename colinds_t::non_const_type>
labels_t graph_mis2_coarsen(const rowmap_t& rowmap, const colinds_t& colinds, typename colinds_t::non_const_value_type& numClusters) {
  if (rowmap.extent(0) <= 1) { numClusters = 0; return labels_t(); }   // there are no vertices to label
  return Impl::mis2_labels<rowmap_t, colinds_t, labels_t>(rowmap, colinds, 0, numClusters);
}

template <typename device_t, typename rowmap_t, typename colinds_t, typename labels_t = typename colinds_t::non_const_type>
labels_t graph_mis2_aggregate(const rowmap_t& rowmap, const colinds_t& colinds, typename colinds_t::non_const_value_type& numAggregates) {
  if (rowmap.extent(0) <= 1) { numAggregates = 0; return labels_t(); }
  return Impl::mis2_labels<rowmap_t, colinds_t, labels_t>(rowmap, colinds, 1, numAggregates);
}

inline const char* mis2_algorithm_name(MIS2_Algorithm algo) {
  switch (algo) {
    case MIS2_QUALITY: return "MIS2_QUALITY";
    case MIS2_FAST: return "MIS2_FAST";
  }
  return "*** Invalid MIS2 algo enum value.\n";
}

// For backward compatibility
namespace Experimental {
template <typename device_t, typename rowmap_t, typename colinds_t, typename lno_view_t = typename colinds_t::non_const_type>
[[deprecated]] lno_view_t graph_d2_mis(const rowmap_t& rowmap, const colinds_t& colinds, MIS2_Algorithm algo = MIS2_FAST) {
  return KokkosGraph::graph_d2_mis<device_t, rowmap_t, colinds_t, lno_view_t>(rowmap, colinds, algo);
}
template <typename device_t, typename rowmap_t, typename colinds_t, typename labels_t = typename colinds_t::non_const_type>
[[deprecated]] labels_t graph_mis2_coarsen(const rowmap_t& rowmap, const colinds_t& colinds, typename colinds_t::non_const_value_type& numClusters) {
  return KokkosGraph::graph_mis2_coarsen<device_t, rowmap_t, colinds_t, labels_t>(rowmap, colinds, numClusters);
}
template <typename device_t, typename rowmap_t, typename colinds_t, typename labels_t = typename colinds_t::non_const_type>
[[deprecated]] labels_t graph_mis2_aggregate(const rowmap_t& rowmap, const colinds_t& colinds, typename colinds_t::non_const_value_type& numAggregates) {
  return KokkosGraph::graph_mis2_aggregate<device_t, rowmap_t, colinds_t, labels_t>(rowmap, colinds, numAggregates);
}
[[deprecated]] inline const char* mis2_algorithm_name(MIS2_Algorithm algo) { return KokkosGraph::mis2_algorithm_name(algo); }
}  // namespace Experimental

}  // namespace KokkosGraph
