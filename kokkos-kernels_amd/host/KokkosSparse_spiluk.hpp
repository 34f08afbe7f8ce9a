// KokkosSparse::spiluk_symbolic / spiluk_numeric -- reference: sparse/src/KokkosSparse_spiluk.hpp:40-197 (symbolic), :197-415
// (numeric), :417-436 (the deprecated KokkosSparse::Experimental:: names that forward).  Kept: argument order, the static_asserts and
// their texts, the run-time checks and their texts (fill_lev, "spiluk_symbolic must be called before spiluk_numeric", the extents of
// L_entries / U_entries), "the handle must carry an SPILUK sub-handle".  Impl::SPILUK_SYMBOLIC / SPILUK_NUMERIC are replaced by the two
// C-ABI calls, on the handle's execution space.  nstreams is accepted and unused (the level sets are not chunked here).
// Not here: spiluk_numeric_streams (:438-), the block (BSR) variant.
#pragma once
#include "KokkosKernels_Handle.hpp"

namespace KokkosSparse {

#define KOKKOSKERNELS_SPILUK_SAME_TYPE(A, B) \
  std::is_same<typename std::remove_const<A>::type, typename std::remove_const<B>::type>::value

template <typename KernelHandle, typename ARowMapType, typename AEntriesType, typename LRowMapType, typename LEntriesType,
          typename URowMapType, typename UEntriesType>
void spiluk_symbolic(KernelHandle* handle, typename KernelHandle::const_nnz_lno_t fill_lev, ARowMapType& A_rowmap, AEntriesType& A_entries,
                     LRowMapType& L_rowmap, LEntriesType& L_entries, URowMapType& U_rowmap, UEntriesType& U_entries, int /*nstreams*/ = 1) {
  typedef typename KernelHandle::size_type size_type;
  typedef typename KernelHandle::nnz_lno_t ordinal_type;
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename ARowMapType::non_const_value_type, size_type),
                "spiluk_symbolic: A size_type must match KernelHandle "
                "size_type (const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename AEntriesType::non_const_value_type, ordinal_type),
                "spiluk_symbolic: A entry type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename LRowMapType::non_const_value_type, size_type),
                "spiluk_symbolic: L size_type must match KernelHandle "
                "size_type (const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename LEntriesType::non_const_value_type, ordinal_type),
                "spiluk_symbolic: L entry type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename URowMapType::non_const_value_type, size_type),
                "spiluk_symbolic: U size_type must match KernelHandle "
                "size_type (const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename UEntriesType::non_const_value_type, ordinal_type),
                "spiluk_symbolic: U entry type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(Kokkos::is_view<ARowMapType>::value, "spiluk_symbolic: A_rowmap is not a Kokkos::View.");
  static_assert(Kokkos::is_view<AEntriesType>::value, "spiluk_symbolic: A_entries is not a Kokkos::View.");
  static_assert(Kokkos::is_view<LRowMapType>::value, "spiluk_symbolic: L_rowmap is not a Kokkos::View.");
  static_assert(Kokkos::is_view<LEntriesType>::value, "spiluk_symbolic: L_entries is not a Kokkos::View.");
  static_assert(Kokkos::is_view<URowMapType>::value, "spiluk_symbolic: U_rowmap is not a Kokkos::View.");
  static_assert(Kokkos::is_view<UEntriesType>::value, "spiluk_symbolic: U_entries is not a Kokkos::View.");
  static_assert((int)LRowMapType::rank() == (int)ARowMapType::rank(), "spiluk_symbolic: The ranks of L_rowmap and A_rowmap do not match.");
  static_assert((int)LEntriesType::rank() == (int)AEntriesType::rank(), "spiluk_symbolic: The ranks of L_entries and A_entries do not match.");
  static_assert((int)LRowMapType::rank() == (int)URowMapType::rank(), "spiluk_symbolic: The ranks of L_rowmap and U_rowmap do not match.");
  static_assert((int)LEntriesType::rank() == (int)UEntriesType::rank(), "spiluk_symbolic: The ranks of L_entries and U_entries do not match.");
  static_assert(LRowMapType::rank() == 1, "spiluk_symbolic: A_rowmap, L_rowmap and U_rowmap must all have rank 1.");
  static_assert(LEntriesType::rank() == 1,
                "spiluk_symbolic: A_entries, L_entries and U_entries must all "
                "have rank 1.");
  static_assert(std::is_same<typename LRowMapType::value_type, typename LRowMapType::non_const_value_type>::value,
                "spiluk_symbolic: The output L_rowmap must be nonconst.");
  static_assert(std::is_same<typename LEntriesType::value_type, typename LEntriesType::non_const_value_type>::value,
                "spiluk_symbolic: The output L_entries must be nonconst.");
  static_assert(std::is_same<typename URowMapType::value_type, typename URowMapType::non_const_value_type>::value,
                "spiluk_symbolic: The output U_rowmap must be nonconst.");
  static_assert(std::is_same<typename UEntriesType::value_type, typename UEntriesType::non_const_value_type>::value,
                "spiluk_symbolic: The output U_entries must be nonconst.");
  static_assert(std::is_same<typename LRowMapType::device_type, typename ARowMapType::device_type>::value,
                "spiluk_symbolic: Views LRowMapType and ARowMapType have "
                "different device_types.");
  static_assert(std::is_same<typename LEntriesType::device_type, typename AEntriesType::device_type>::value,
                "spiluk_symbolic: Views LEntriesType and AEntriesType have "
                "different device_types.");
  static_assert(std::is_same<typename LRowMapType::device_type, typename URowMapType::device_type>::value,
                "spiluk_symbolic: Views LRowMapType and URowMapType have "
                "different device_types.");
  static_assert(std::is_same<typename LEntriesType::device_type, typename UEntriesType::device_type>::value,
                "spiluk_symbolic: Views LEntriesType and UEntriesType have "
                "different device_types.");
  static_assert(std::is_same<typename LRowMapType::device_type::execution_space, typename KernelHandle::SPILUKHandleType::execution_space>::value,
                "spiluk_symbolic: KernelHandle and Views have different execution "
                "spaces.");
  static_assert(std::is_same<typename LEntriesType::device_type::execution_space, typename KernelHandle::SPILUKHandleType::execution_space>::value,
                "spiluk_symbolic: KernelHandle and Views have different execution "
                "spaces.");
  static_assert(std::is_same<typename LRowMapType::device_type, typename LEntriesType::device_type>::value,
                "spiluk_symbolic: rowmap and entries have different device types.");
  static_assert(std::is_same<ordinal_type, int>::value, "kkamd: ordinals must be int32");
  if (fill_lev < 0)
    throw std::runtime_error("KokkosSparse::Experimental::spiluk_symbolic: fill_lev: " + std::to_string(fill_lev) + ". Valid value is >= 0.");
  auto* sh = handle->get_spiluk_handle();
  if (!sh) throw std::invalid_argument("KokkosSparse::spiluk_symbolic: the given KernelHandle does not have an SPILUK handle associated with it.");
  const int64_t nrows = A_rowmap.extent(0) ? (int64_t)A_rowmap.extent(0) - 1 : 0;
  if ((int64_t)L_rowmap.extent(0) != nrows + 1 || (int64_t)U_rowmap.extent(0) != nrows + 1)
    throw std::runtime_error("KokkosSparse::spiluk_symbolic: L_rowmap and U_rowmap must have A_rowmap's extent " + std::to_string(nrows + 1));
  typename KernelHandle::HandleExecSpace space;
  Kokkos::Profiling::pushRegion("KokkosSparse::spiluk_symbolic[KKAMD]");
  const int rc = kkamd_spiluk_symbolic(sh->native(), (int)fill_lev, nrows, A_rowmap.data(), A_entries.data(), (void*)L_rowmap.data(), L_entries.data(),
                                       (int64_t)L_entries.extent(0), (void*)U_rowmap.data(), U_entries.data(), (int64_t)U_entries.extent(0),
                                       Impl::kkamd_offset<size_type>::value, reinterpret_cast<kkamd_stream_t>(space.hip_stream()));
  Kokkos::Profiling::popRegion();
  Impl::kkamd_check(rc);
  sh->symbolic_done();
}

template <typename KernelHandle, typename ARowMapType, typename AEntriesType, typename AValuesType, typename LRowMapType, typename LEntriesType,
          typename LValuesType, typename URowMapType, typename UEntriesType, typename UValuesType>
void spiluk_numeric(KernelHandle* handle, typename KernelHandle::const_nnz_lno_t fill_lev, ARowMapType& A_rowmap, AEntriesType& A_entries,
                    AValuesType& A_values, LRowMapType& L_rowmap, LEntriesType& L_entries, LValuesType& L_values, URowMapType& U_rowmap,
                    UEntriesType& U_entries, UValuesType& U_values) {
  typedef typename KernelHandle::size_type size_type;
  typedef typename KernelHandle::nnz_lno_t ordinal_type;
  typedef typename KernelHandle::nnz_scalar_t scalar_type;
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename ARowMapType::non_const_value_type, size_type),
                "spiluk_numeric: A size_type must match KernelHandle size_type "
                "(const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename AEntriesType::non_const_value_type, ordinal_type),
                "spiluk_numeric: A entry type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename AValuesType::value_type, scalar_type),
                "spiluk_numeric: A scalar type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename LRowMapType::non_const_value_type, size_type),
                "spiluk_numeric: L size_type must match KernelHandle size_type "
                "(const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename LEntriesType::non_const_value_type, ordinal_type),
                "spiluk_numeric: L entry type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename LValuesType::value_type, scalar_type),
                "spiluk_numeric: L scalar type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename URowMapType::non_const_value_type, size_type),
                "spiluk_numeric: U size_type must match KernelHandle size_type "
                "(const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename UEntriesType::non_const_value_type, ordinal_type),
                "spiluk_numeric: U entry type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_SPILUK_SAME_TYPE(typename UValuesType::value_type, scalar_type),
                "spiluk_numeric: U scalar type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(Kokkos::is_view<ARowMapType>::value, "spiluk_numeric: A_rowmap is not a Kokkos::View.");
  static_assert(Kokkos::is_view<AEntriesType>::value, "spiluk_numeric: A_entries is not a Kokkos::View.");
  static_assert(Kokkos::is_view<AValuesType>::value, "spiluk_numeric: A_values is not a Kokkos::View.");
  static_assert(Kokkos::is_view<LRowMapType>::value, "spiluk_numeric: L_rowmap is not a Kokkos::View.");
  static_assert(Kokkos::is_view<LEntriesType>::value, "spiluk_numeric: L_entries is not a Kokkos::View.");
  static_assert(Kokkos::is_view<LValuesType>::value, "spiluk_numeric: L_values is not a Kokkos::View.");
  static_assert(Kokkos::is_view<URowMapType>::value, "spiluk_numeric: U_rowmap is not a Kokkos::View.");
  static_assert(Kokkos::is_view<UEntriesType>::value, "spiluk_numeric: U_entries is not a Kokkos::View.");
  static_assert(Kokkos::is_view<UValuesType>::value, "spiluk_numeric: U_values is not a Kokkos::View.");
  static_assert((int)LRowMapType::rank() == (int)ARowMapType::rank(), "spiluk_numeric: The ranks of L_rowmap and A_rowmap do not match.");
  static_assert((int)LEntriesType::rank() == (int)AEntriesType::rank(), "spiluk_numeric: The ranks of L_entries and A_entries do not match.");
  static_assert((int)LValuesType::rank() == (int)AValuesType::rank(), "spiluk_numeric: The ranks of L_values and A_values do not match.");
  static_assert((int)LRowMapType::rank() == (int)URowMapType::rank(), "spiluk_numeric: The ranks of L_rowmap and U_rowmap do not match.");
  static_assert((int)LEntriesType::rank() == (int)UEntriesType::rank(), "spiluk_numeric: The ranks of L_entries and U_entries do not match.");
  static_assert((int)LValuesType::rank() == (int)UValuesType::rank(), "spiluk_numeric: The ranks of L_values and U_values do not match.");
  static_assert(LRowMapType::rank() == 1, "spiluk_numeric: A_rowmap, L_rowmap and U_rowmap must all have rank 1.");
  static_assert(LEntriesType::rank() == 1,
                "spiluk_numeric: A_entries, L_entries and U_entries must all "
                "have rank 1.");
  static_assert(LValuesType::rank() == 1, "spiluk_numeric: A_values, L_values and U_values must all have rank 1.");
  static_assert(std::is_same<typename LEntriesType::value_type, typename LEntriesType::non_const_value_type>::value,
                "spiluk_numeric: The output L_entries must be nonconst.");
  static_assert(std::is_same<typename LValuesType::value_type, typename LValuesType::non_const_value_type>::value,
                "spiluk_numeric: The output L_values must be nonconst.");
  static_assert(std::is_same<typename UEntriesType::value_type, typename UEntriesType::non_const_value_type>::value,
                "spiluk_numeric: The output U_entries must be nonconst.");
  static_assert(std::is_same<typename UValuesType::value_type, typename UValuesType::non_const_value_type>::value,
                "spiluk_numeric: The output U_values must be nonconst.");
  static_assert(std::is_same<typename LRowMapType::device_type, typename ARowMapType::device_type>::value,
                "spiluk_numeric: Views LRowMapType and ARowMapType have "
                "different device_types.");
  static_assert(std::is_same<typename LEntriesType::device_type, typename AEntriesType::device_type>::value,
                "spiluk_numeric: Views LEntriesType and AEntriesType have "
                "different device_types.");
  static_assert(std::is_same<typename LValuesType::device_type, typename AValuesType::device_type>::value,
                "spiluk_numeric: Views LValuesType and AValuesType have "
                "different device_types.");
  static_assert(std::is_same<typename LRowMapType::device_type, typename URowMapType::device_type>::value,
                "spiluk_numeric: Views LRowMapType and URowMapType have "
                "different device_types.");
  static_assert(std::is_same<typename LEntriesType::device_type, typename UEntriesType::device_type>::value,
                "spiluk_numeric: Views LEntriesType and UEntriesType have "
                "different device_types.");
  static_assert(std::is_same<typename LValuesType::device_type, typename UValuesType::device_type>::value,
                "spiluk_numeric: Views LValuesType and UValuesType have "
                "different device_types.");
  static_assert(std::is_same<typename LRowMapType::device_type::execution_space, typename KernelHandle::SPILUKHandleType::execution_space>::value,
                "spiluk_numeric: KernelHandle and Views have different execution "
                "spaces.");
  static_assert(std::is_same<typename LEntriesType::device_type::execution_space, typename KernelHandle::SPILUKHandleType::execution_space>::value,
                "spiluk_numeric: KernelHandle and Views have different execution "
                "spaces.");
  static_assert(std::is_same<typename LValuesType::device_type::execution_space, typename KernelHandle::SPILUKHandleType::execution_space>::value,
                "spiluk_numeric: KernelHandle and Views have different execution "
                "spaces.");
  static_assert(std::is_same<typename LRowMapType::device_type, typename LEntriesType::device_type>::value,
                "spiluk_numeric: rowmap and entries have different device types.");
  static_assert(std::is_same<typename LRowMapType::device_type, typename LValuesType::device_type>::value,
                "spiluk_numeric: rowmap and values have different device types.");
  static_assert(std::is_same<ordinal_type, int>::value, "kkamd: ordinals must be int32");
  if (fill_lev < 0)
    throw std::runtime_error("KokkosSparse::Experimental::spiluk_numeric: fill_lev: " + std::to_string(fill_lev) + ". Valid value is >= 0.");
  auto* sh = handle->get_spiluk_handle();
  if (!sh) throw std::invalid_argument("KokkosSparse::spiluk_numeric: the given KernelHandle does not have an SPILUK handle associated with it.");
  if (!sh->is_symbolic_complete())
    throw std::runtime_error("KokkosSparse::Experimental::spiluk_numeric: spiluk_symbolic must be called before spiluk_numeric.");
  const int64_t nrows = A_rowmap.extent(0) ? (int64_t)A_rowmap.extent(0) - 1 : 0;
  if ((int64_t)L_values.extent(0) < sh->get("nnzL") || (int64_t)U_values.extent(0) < sh->get("nnzU") ||
      (int64_t)L_entries.extent(0) < sh->get("nnzL") || (int64_t)U_entries.extent(0) < sh->get("nnzU"))
    throw std::runtime_error("KokkosSparse::spiluk_numeric: the views of L or U are shorter than nnzL / nnzU of the symbolic phase");
  typename KernelHandle::HandleExecSpace space;
  Kokkos::Profiling::pushRegion("KokkosSparse::spiluk_numeric[KKAMD]");
  const int rc = kkamd_spiluk_numeric(sh->native(), (int)fill_lev, nrows, A_rowmap.data(), A_entries.data(), A_values.data(), L_rowmap.data(),
                                      L_entries.data(), (void*)L_values.data(), U_rowmap.data(), U_entries.data(), (void*)U_values.data(),
                                      Impl::kkamd_offset<size_type>::value, Impl::kkamd_scalar<scalar_type>::value,
                                      reinterpret_cast<kkamd_stream_t>(space.hip_stream()));
  Kokkos::Profiling::popRegion();
  Impl::kkamd_check(rc);
}

namespace Experimental {

template <typename KernelHandle, typename ARowMapType, typename AEntriesType, typename LRowMapType, typename LEntriesType,
          typename URowMapType, typename UEntriesType>
[[deprecated("spiluk_symbolic was promoted out of Experimental, please use KokkosSparse::spiluk_symbolic instead.")]] void spiluk_symbolic(
    KernelHandle* handle, typename KernelHandle::const_nnz_lno_t fill_lev, ARowMapType& A_rowmap, AEntriesType& A_entries, LRowMapType& L_rowmap,
    LEntriesType& L_entries, URowMapType& U_rowmap, UEntriesType& U_entries, int nstreams = 1) {
  KokkosSparse::spiluk_symbolic(handle, fill_lev, A_rowmap, A_entries, L_rowmap, L_entries, U_rowmap, U_entries, nstreams);
}

template <typename KernelHandle, typename ARowMapType, typename AEntriesType, typename AValuesType, typename LRowMapType, typename LEntriesType,
          typename LValuesType, typename URowMapType, typename UEntriesType, typename UValuesType>
[[deprecated("spiluk_numeric was promoted out of Experimental, please use KokkosSparse::spiluk_numeric instead.")]] void spiluk_numeric(
    KernelHandle* handle, typename KernelHandle::const_nnz_lno_t fill_lev, ARowMapType& A_rowmap, AEntriesType& A_entries, AValuesType& A_values,
    LRowMapType& L_rowmap, LEntriesType& L_entries, LValuesType& L_values, URowMapType& U_rowmap, UEntriesType& U_entries, UValuesType& U_values) {
  KokkosSparse::spiluk_numeric(handle, fill_lev, A_rowmap, A_entries, A_values, L_rowmap, L_entries, L_values, U_rowmap, U_entries, U_values);
}

}  // namespace Experimental
}  // namespace KokkosSparse

#undef KOKKOSKERNELS_SPILUK_SAME_TYPE
