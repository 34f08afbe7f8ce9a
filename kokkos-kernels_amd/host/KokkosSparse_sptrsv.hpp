// KokkosSparse::sptrsv_symbolic / sptrsv_solve -- reference: sparse/src/KokkosSparse_sptrsv.hpp:54-122 (symbolic, with and without an
// execution space), :268-411 (solve), :706-750 (the deprecated KokkosSparse::Experimental:: names that forward).  Kept: argument order,
// the static_asserts and their texts, rank-1 b and x, "the handle must carry an SPTRSV sub-handle".  Impl::SPTRSV_SYMBOLIC /
// SPTRSV_SOLVE are replaced by the two C-ABI calls, on the execution space's stream.  The symbolic overloads that take values
// (:139-253, used by the cuSPARSE and supernodal paths) forward to the graph-only analysis.
#pragma once
#include "KokkosKernels_Handle.hpp"

namespace KokkosSparse {

#define KOKKOSKERNELS_SPTRSV_SAME_TYPE(A, B) \
  std::is_same<typename std::remove_const<A>::type, typename std::remove_const<B>::type>::value

template <typename ExecutionSpace, typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_>
void sptrsv_symbolic(const ExecutionSpace& space, KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries) {
  typedef typename KernelHandle::size_type size_type;
  typedef typename KernelHandle::nnz_lno_t ordinal_type;
  static_assert(KOKKOSKERNELS_SPTRSV_SAME_TYPE(typename lno_row_view_t_::non_const_value_type, size_type),
                "sptrsv_symbolic: A size_type must match KernelHandle "
                "size_type (const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPTRSV_SAME_TYPE(typename lno_nnz_view_t_::non_const_value_type, ordinal_type),
                "sptrsv_symbolic: A entry type must match KernelHandle entry type (aka "
                "nnz_lno_t, and const doesn't matter)");
  static_assert(std::is_same<ordinal_type, int>::value, "kkamd: ordinals must be int32");
  auto* sh = handle->get_sptrsv_handle();
  if (!sh) throw std::invalid_argument("KokkosSparse::sptrsv_symbolic: the given KernelHandle does not have an SPTRSV handle associated with it.");
  if (rowmap.extent(0) == 0 && sh->get_nrows() != 0) throw std::runtime_error("KokkosSparse::sptrsv_symbolic: rowmap is empty");
  const int64_t nrows = rowmap.extent(0) ? (int64_t)rowmap.extent(0) - 1 : 0;
  Kokkos::Profiling::pushRegion("KokkosSparse::sptrsv_symbolic[KKAMD]");
  const int rc = kkamd_sptrsv_symbolic(sh->native(), nrows, rowmap.data(), entries.data(), Impl::kkamd_offset<size_type>::value,
                                       reinterpret_cast<kkamd_stream_t>(space.hip_stream()));
  Kokkos::Profiling::popRegion();
  Impl::kkamd_check(rc);
}

template <typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_>
void sptrsv_symbolic(KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries) {
  using ExecutionSpace = typename KernelHandle::HandleExecSpace;
  auto my_exec_space   = ExecutionSpace();
  sptrsv_symbolic(my_exec_space, handle, rowmap, entries);
}

template <typename ExecutionSpace, typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_, typename scalar_nnz_view_t_>
void sptrsv_symbolic(ExecutionSpace& space, KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries, scalar_nnz_view_t_ /*values*/) {
  static_assert(KOKKOSKERNELS_SPTRSV_SAME_TYPE(typename scalar_nnz_view_t_::value_type, typename KernelHandle::nnz_scalar_t),
                "sptrsv_symbolic: A scalar type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  sptrsv_symbolic(static_cast<const ExecutionSpace&>(space), handle, rowmap, entries);
}

template <typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_, typename scalar_nnz_view_t_>
void sptrsv_symbolic(KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values) {
  using ExecutionSpace = typename KernelHandle::HandleExecSpace;
  auto my_exec_space   = ExecutionSpace();
  sptrsv_symbolic(my_exec_space, handle, rowmap, entries, values);
}

template <typename ExecutionSpace, typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_, typename scalar_nnz_view_t_,
          class BType, class XType>
void sptrsv_solve(ExecutionSpace& space, KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values,
                  BType b, XType x) {
  typedef typename KernelHandle::size_type size_type;
  typedef typename KernelHandle::nnz_lno_t ordinal_type;
  typedef typename KernelHandle::nnz_scalar_t scalar_type;
  static_assert(std::is_same<ExecutionSpace, typename KernelHandle::HandleExecSpace>::value,
                "sptrsv solve: ExecutionSpace and HandleExecSpace need to match");
  static_assert(KOKKOSKERNELS_SPTRSV_SAME_TYPE(typename lno_row_view_t_::non_const_value_type, size_type),
                "sptrsv_solve: A size_type must match KernelHandle size_type "
                "(const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPTRSV_SAME_TYPE(typename lno_nnz_view_t_::non_const_value_type, ordinal_type),
                "sptrsv_solve: A entry type must match KernelHandle entry type (aka "
                "nnz_lno_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPTRSV_SAME_TYPE(typename scalar_nnz_view_t_::value_type, scalar_type),
                "sptrsv_solve: A scalar type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(Kokkos::is_view<BType>::value, "sptrsv: b is not a Kokkos::View.");
  static_assert(Kokkos::is_view<XType>::value, "sptrsv: x is not a Kokkos::View.");
  static_assert((int)BType::rank() == (int)XType::rank(), "sptrsv: The ranks of b and x do not match.");
  static_assert(BType::rank() == 1, "sptrsv: b and x must both either have rank 1.");
  static_assert(std::is_same<typename XType::value_type, typename XType::non_const_value_type>::value,
                "sptrsv: The output x must be nonconst.");
  static_assert(std::is_same<typename BType::device_type, typename XType::device_type>::value,
                "sptrsv: Views BType and XType have different device_types.");
  static_assert(std::is_same<typename BType::device_type::execution_space, typename KernelHandle::SPTRSVHandleType::execution_space>::value,
                "sptrsv: KernelHandle and Views have different execution spaces.");
  static_assert(std::is_same<typename lno_row_view_t_::device_type, typename lno_nnz_view_t_::device_type>::value,
                "sptrsv: rowmap and entries have different device types.");
  static_assert(std::is_same<typename lno_row_view_t_::device_type, typename scalar_nnz_view_t_::device_type>::value,
                "sptrsv: rowmap and values have different device types.");
  static_assert(KOKKOSKERNELS_SPTRSV_SAME_TYPE(typename BType::value_type, scalar_type) &&
                    KOKKOSKERNELS_SPTRSV_SAME_TYPE(typename XType::value_type, scalar_type),
                "kkamd: b and x must have the scalar type of A (type pairs (double, double) and (float, float))");
  auto* sh = handle->get_sptrsv_handle();
  if (!sh) throw std::invalid_argument("KokkosSparse::sptrsv_solve: the given KernelHandle does not have an SPTRSV handle associated with it.");
  const int64_t nrows = rowmap.extent(0) ? (int64_t)rowmap.extent(0) - 1 : 0;
  if ((int64_t)b.extent(0) != nrows || (int64_t)x.extent(0) != nrows)
    throw std::runtime_error("KokkosSparse::sptrsv_solve: Dimensions do not match: A: " + std::to_string(nrows) + " x " + std::to_string(nrows) +
                             ", b: " + std::to_string(b.extent(0)) + ", x: " + std::to_string(x.extent(0)));
  if (nrows > 1 && (b.stride(0) != 1 || x.stride(0) != 1)) throw std::runtime_error("KokkosSparse::sptrsv_solve: b and x must be contiguous");
  Kokkos::Profiling::pushRegion("KokkosSparse::sptrsv_solve[KKAMD]");
  const int rc = kkamd_sptrsv_solve(sh->native(), nrows, rowmap.data(), entries.data(), values.data(), b.data(), (void*)x.data(),
                                    Impl::kkamd_offset<size_type>::value, Impl::kkamd_scalar<scalar_type>::value,
                                    reinterpret_cast<kkamd_stream_t>(space.hip_stream()));
  Kokkos::Profiling::popRegion();
  Impl::kkamd_check(rc);
}

template <typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_, typename scalar_nnz_view_t_, class BType, class XType>
void sptrsv_solve(KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values, BType b, XType x) {
  using ExecutionSpace = typename KernelHandle::HandleExecSpace;
  auto my_exec_space   = ExecutionSpace();
  sptrsv_solve(my_exec_space, handle, rowmap, entries, values, b, x);
}

namespace Experimental {

template <typename ExecutionSpace, typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_>
[[deprecated("sptrsv_symbolic was promoted out of Experimental, please use KokkosSparse::sptrsv_symbolic instead.")]] void
sptrsv_symbolic(const ExecutionSpace& space, KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries) {
  KokkosSparse::sptrsv_symbolic(space, handle, rowmap, entries);
}

template <typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_>
[[deprecated("sptrsv_symbolic was promoted out of Experimental, please use KokkosSparse::sptrsv_symbolic instead.")]] void
sptrsv_symbolic(KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries) {
  KokkosSparse::sptrsv_symbolic(handle, rowmap, entries);
}

template <typename ExecutionSpace, typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_, typename scalar_nnz_view_t_>
[[deprecated("sptrsv_symbolic was promoted out of Experimental, please use KokkosSparse::sptrsv_symbolic instead.")]] void
sptrsv_symbolic(ExecutionSpace& space, KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values) {
  KokkosSparse::sptrsv_symbolic(space, handle, rowmap, entries, values);
}

template <typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_, typename scalar_nnz_view_t_>
[[deprecated("sptrsv_symbolic was promoted out of Experimental, please use KokkosSparse::sptrsv_symbolic instead.")]] void
sptrsv_symbolic(KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values) {
  KokkosSparse::sptrsv_symbolic(handle, rowmap, entries, values);
}

template <typename ExecutionSpace, typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_, typename scalar_nnz_view_t_,
          class BType, class XType>
[[deprecated("sptrsv_solve was promoted out of Experimental, please use KokkosSparse::sptrsv_symbolic instead.")]] void
sptrsv_solve(ExecutionSpace& space, KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values, BType b,
             XType x) {
  KokkosSparse::sptrsv_solve(space, handle, rowmap, entries, values, b, x);
}

template <typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_, typename scalar_nnz_view_t_, class BType, class XType>
[[deprecated("sptrsv_solve was promoted out of Experimental, please use KokkosSparse::sptrsv_symbolic instead.")]] void
sptrsv_solve(KernelHandle* handle, lno_row_view_t_ rowmap, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values, BType b, XType x) {
  KokkosSparse::sptrsv_solve(handle, rowmap, entries, values, b, x);
}

}  // namespace Experimental
}  // namespace KokkosSparse

#undef KOKKOSKERNELS_SPTRSV_SAME_TYPE
