// KokkosSparse::Experimental::par_ilut_symbolic / par_ilut_numeric -- reference: sparse/src/KokkosSparse_par_ilut.hpp:76-190 (symbolic),
// :207-380 (numeric).  Kept: argument order, the static_asserts and their texts, the run-time checks and their texts ("par_ilut_symbolic
// must be called before par_ilut_numeric", the row map sizes).  Impl::PAR_ILUT_SYMBOLIC / PAR_ILUT_NUMERIC are replaced by the C-ABI calls
// on the handle's execution space.  As in the reference the numeric phase resizes the caller's six views of L and U: their final extents are
// the factors' sizes.  "A is not sorted" is reported by the symbolic phase here, naming the row (include/kkamd.h).
// Not here: async_update = true (recorded, without effect, as in the reference), BSR, complex scalars.
#pragma once
#include "KokkosKernels_Handle.hpp"

namespace KokkosSparse { namespace Experimental {

#define KKAMD_PARILUT_SAME(A, B) std::is_same<typename std::remove_const<A>::type, typename std::remove_const<B>::type>::value
#define KKAMD_PARILUT_NONCONST(V) std::is_same<typename V::value_type, typename V::non_const_value_type>::value
#define KKAMD_PARILUT_SAME_DEV(V, W) std::is_same<typename V::device_type, typename W::device_type>::value
#define KKAMD_PARILUT_EXEC(V, KH) \
  std::is_same<typename V::device_type::execution_space, typename KH::PAR_ILUTHandleType::execution_space>::value

template <typename KernelHandle, typename ARowMapType, typename AEntriesType, typename LRowMapType, typename URowMapType>
void par_ilut_symbolic(KernelHandle* handle, ARowMapType& A_rowmap, AEntriesType& A_entries, LRowMapType& L_rowmap, URowMapType& U_rowmap) {
  using size_type    = typename KernelHandle::size_type;
  using ordinal_type = typename KernelHandle::nnz_lno_t;
  static_assert(KKAMD_PARILUT_SAME(typename ARowMapType::non_const_value_type, size_type),
                "par_ilut_symbolic: A size_type must match KernelHandle "
                "size_type (const doesn't matter)");
  static_assert(KKAMD_PARILUT_SAME(typename AEntriesType::non_const_value_type, ordinal_type),
                "par_ilut_symbolic: A entry type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KKAMD_PARILUT_SAME(typename LRowMapType::non_const_value_type, size_type),
                "par_ilut_symbolic: L size_type must match KernelHandle "
                "size_type (const doesn't matter)");
  static_assert(KKAMD_PARILUT_SAME(typename URowMapType::non_const_value_type, size_type),
                "par_ilut_symbolic: U size_type must match KernelHandle "
                "size_type (const doesn't matter)");
  static_assert(Kokkos::is_view<ARowMapType>::value, "par_ilut_symbolic: A_rowmap is not a Kokkos::View.");
  static_assert(Kokkos::is_view<AEntriesType>::value, "par_ilut_symbolic: A_entries is not a Kokkos::View.");
  static_assert(Kokkos::is_view<LRowMapType>::value, "par_ilut_symbolic: L_rowmap is not a Kokkos::View.");
  static_assert(Kokkos::is_view<URowMapType>::value, "par_ilut_symbolic: U_rowmap is not a Kokkos::View.");
  static_assert((int)LRowMapType::rank() == (int)ARowMapType::rank(), "par_ilut_symbolic: The ranks of L_rowmap and A_rowmap do not match.");
  static_assert((int)LRowMapType::rank() == (int)URowMapType::rank(), "par_ilut_symbolic: The ranks of L_rowmap and U_rowmap do not match.");
  static_assert(LRowMapType::rank() == 1,
                "par_ilut_symbolic: A_rowmap, L_rowmap and U_rowmap must all "
                "have rank 1.");
  static_assert(KKAMD_PARILUT_NONCONST(LRowMapType), "par_ilut_symbolic: The output L_rowmap must be nonconst.");
  static_assert(KKAMD_PARILUT_NONCONST(URowMapType), "par_ilut_symbolic: The output U_rowmap must be nonconst.");
  static_assert(KKAMD_PARILUT_SAME_DEV(LRowMapType, ARowMapType),
                "par_ilut_symbolic: Views LRowMapType and ARowMapType have "
                "different device_types.");
  static_assert(KKAMD_PARILUT_SAME_DEV(LRowMapType, URowMapType),
                "par_ilut_symbolic: Views LRowMapType and URowMapType have "
                "different device_types.");
  static_assert(KKAMD_PARILUT_EXEC(LRowMapType, KernelHandle),
                "par_ilut_symbolic: KernelHandle and Views have different execution "
                "spaces.");
  static_assert(std::is_same<ordinal_type, int>::value, "kkamd: ordinals must be int32");
  auto* ih = handle->get_par_ilut_handle();
  if (!ih) throw std::invalid_argument("KokkosSparse::par_ilut_symbolic: the given KernelHandle does not have a PAR_ILUT handle associated with it.");
  if (A_rowmap.extent(0) != 0) {
    if (A_rowmap.extent(0) != L_rowmap.extent(0)) throw std::runtime_error("L row map size does not match A row map");
    if (A_rowmap.extent(0) != U_rowmap.extent(0)) throw std::runtime_error("U row map size does not match A row map");
  }
  const int64_t nrows = A_rowmap.extent(0) ? (int64_t)A_rowmap.extent(0) - 1 : 0;
  typename KernelHandle::HandleExecSpace space;
  if (A_rowmap.extent(0) == 0) {   // no row map at all: the empty matrix (the reference's zero-row test passes views of extent 0)
    Kokkos::View<size_type*, typename ARowMapType::device_type> zero("par_ilut zero row map", 1);
    if (L_rowmap.extent(0) == 0) Kokkos::resize(L_rowmap, 1);
    if (U_rowmap.extent(0) == 0) Kokkos::resize(U_rowmap, 1);
    KokkosSparse::Impl::kkamd_check(kkamd_par_ilut_symbolic(ih->native(), 0, zero.data(), A_entries.data(), (void*)L_rowmap.data(), (void*)U_rowmap.data(),
                                                            KokkosSparse::Impl::kkamd_offset<size_type>::value,
                                                            reinterpret_cast<kkamd_stream_t>(space.hip_stream())));
    ih->set_symbolic_complete();
    return;
  }
  Kokkos::Profiling::pushRegion("KokkosSparse::par_ilut_symbolic[KKAMD]");
  const int rc = kkamd_par_ilut_symbolic(ih->native(), nrows, A_rowmap.data(), A_entries.data(), (void*)L_rowmap.data(), (void*)U_rowmap.data(),
                                         KokkosSparse::Impl::kkamd_offset<size_type>::value, reinterpret_cast<kkamd_stream_t>(space.hip_stream()));
  Kokkos::Profiling::popRegion();
  KokkosSparse::Impl::kkamd_check(rc);
  ih->set_symbolic_complete();
}

template <typename KernelHandle, typename ARowMapType, typename AEntriesType, typename AValuesType, typename LRowMapType, typename LEntriesType,
          typename LValuesType, typename URowMapType, typename UEntriesType, typename UValuesType>
void par_ilut_numeric(KernelHandle* handle, ARowMapType& A_rowmap, AEntriesType& A_entries, AValuesType& A_values, LRowMapType& L_rowmap,
                      LEntriesType& L_entries, LValuesType& L_values, URowMapType& U_rowmap, UEntriesType& U_entries, UValuesType& U_values) {
  using size_type    = typename KernelHandle::size_type;
  using ordinal_type = typename KernelHandle::nnz_lno_t;
  using scalar_type  = typename KernelHandle::nnz_scalar_t;
  static_assert(KKAMD_PARILUT_SAME(typename ARowMapType::non_const_value_type, size_type),
                "par_ilut_numeric: A size_type must match KernelHandle size_type "
                "(const doesn't matter)");
  static_assert(KKAMD_PARILUT_SAME(typename AEntriesType::non_const_value_type, ordinal_type),
                "par_ilut_numeric: A entry type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KKAMD_PARILUT_SAME(typename AValuesType::value_type, scalar_type),
                "par_ilut_numeric: A scalar type must match KernelHandle entry "
                "type (aka nnz_scalar_t, and const doesn't matter)");
  static_assert(KKAMD_PARILUT_SAME(typename LRowMapType::non_const_value_type, size_type),
                "par_ilut_numeric: L size_type must match KernelHandle size_type "
                "(const doesn't matter)");
  static_assert(KKAMD_PARILUT_SAME(typename LEntriesType::non_const_value_type, ordinal_type),
                "par_ilut_numeric: L entry type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KKAMD_PARILUT_SAME(typename LValuesType::value_type, scalar_type),
                "par_ilut_numeric: L scalar type must match KernelHandle entry "
                "type (aka nnz_scalar_t, and const doesn't matter)");
  static_assert(KKAMD_PARILUT_SAME(typename URowMapType::non_const_value_type, size_type),
                "par_ilut_numeric: U size_type must match KernelHandle size_type "
                "(const doesn't matter)");
  static_assert(KKAMD_PARILUT_SAME(typename UEntriesType::non_const_value_type, ordinal_type),
                "par_ilut_numeric: U entry type must match KernelHandle entry "
                "type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KKAMD_PARILUT_SAME(typename UValuesType::value_type, scalar_type),
                "par_ilut_numeric: U scalar type must match KernelHandle entry "
                "type (aka nnz_scalar_t, and const doesn't matter)");
  static_assert(Kokkos::is_view<ARowMapType>::value, "par_ilut_numeric: A_rowmap is not a Kokkos::View.");
  static_assert(Kokkos::is_view<AEntriesType>::value, "par_ilut_numeric: A_entries is not a Kokkos::View.");
  static_assert(Kokkos::is_view<AValuesType>::value, "par_ilut_numeric: A_values is not a Kokkos::View.");
  static_assert(Kokkos::is_view<LRowMapType>::value, "par_ilut_numeric: L_rowmap is not a Kokkos::View.");
  static_assert(Kokkos::is_view<LEntriesType>::value, "par_ilut_numeric: L_entries is not a Kokkos::View.");
  static_assert(Kokkos::is_view<LValuesType>::value, "par_ilut_numeric: L_values is not a Kokkos::View.");
  static_assert(Kokkos::is_view<URowMapType>::value, "par_ilut_numeric: U_rowmap is not a Kokkos::View.");
  static_assert(Kokkos::is_view<UEntriesType>::value, "par_ilut_numeric: U_entries is not a Kokkos::View.");
  static_assert(Kokkos::is_view<UValuesType>::value, "par_ilut_numeric: U_values is not a Kokkos::View.");
  static_assert((int)LRowMapType::rank() == (int)ARowMapType::rank(), "par_ilut_numeric: The ranks of L_rowmap and A_rowmap do not match.");
  static_assert((int)LEntriesType::rank() == (int)AEntriesType::rank(), "par_ilut_numeric: The ranks of L_entries and A_entries do not match.");
  static_assert((int)LValuesType::rank() == (int)AValuesType::rank(), "par_ilut_numeric: The ranks of L_values and A_values do not match.");
  static_assert((int)LRowMapType::rank() == (int)URowMapType::rank(), "par_ilut_numeric: The ranks of L_rowmap and U_rowmap do not match.");
  static_assert((int)LEntriesType::rank() == (int)UEntriesType::rank(), "par_ilut_numeric: The ranks of L_entries and U_entries do not match.");
  static_assert((int)LValuesType::rank() == (int)UValuesType::rank(), "par_ilut_numeric: The ranks of L_values and U_values do not match.");
  static_assert(LRowMapType::rank() == 1,
                "par_ilut_numeric: A_rowmap, L_rowmap and U_rowmap must all "
                "have rank 1.");
  static_assert(LEntriesType::rank() == 1,
                "par_ilut_numeric: A_entries, L_entries and U_entries must all "
                "have rank 1.");
  static_assert(LValuesType::rank() == 1,
                "par_ilut_numeric: A_values, L_values and U_values must all "
                "have rank 1.");
  static_assert(KKAMD_PARILUT_NONCONST(LEntriesType), "par_ilut_numeric: The output L_entries must be nonconst.");
  static_assert(KKAMD_PARILUT_NONCONST(LValuesType), "par_ilut_numeric: The output L_values must be nonconst.");
  static_assert(KKAMD_PARILUT_NONCONST(UEntriesType), "par_ilut_numeric: The output U_entries must be nonconst.");
  static_assert(KKAMD_PARILUT_NONCONST(UValuesType), "par_ilut_numeric: The output U_values must be nonconst.");
  static_assert(KKAMD_PARILUT_SAME_DEV(LRowMapType, ARowMapType),
                "par_ilut_numeric: Views LRowMapType and ARowMapType have "
                "different device_types.");
  static_assert(KKAMD_PARILUT_SAME_DEV(LEntriesType, AEntriesType),
                "par_ilut_numeric: Views LEntriesType and AEntriesType have "
                "different device_types.");
  static_assert(KKAMD_PARILUT_SAME_DEV(LValuesType, AValuesType),
                "par_ilut_numeric: Views LValuesType and AValuesType have "
                "different device_types.");
  static_assert(KKAMD_PARILUT_SAME_DEV(LRowMapType, URowMapType),
                "par_ilut_numeric: Views LRowMapType and URowMapType have "
                "different device_types.");
  static_assert(KKAMD_PARILUT_SAME_DEV(LEntriesType, UEntriesType),
                "par_ilut_numeric: Views LEntriesType and UEntriesType have "
                "different device_types.");
  static_assert(KKAMD_PARILUT_SAME_DEV(LValuesType, UValuesType),
                "par_ilut_numeric: Views LValuesType and UValuesType have "
                "different device_types.");
  static_assert(KKAMD_PARILUT_EXEC(LRowMapType, KernelHandle),
                "par_ilut_numeric: KernelHandle and Views have different execution "
                "spaces.");
  static_assert(KKAMD_PARILUT_EXEC(LEntriesType, KernelHandle),
                "par_ilut_numeric: KernelHandle and Views have different execution "
                "spaces.");
  static_assert(KKAMD_PARILUT_EXEC(LValuesType, KernelHandle),
                "par_ilut_numeric: KernelHandle and Views have different execution "
                "spaces.");
  static_assert(KKAMD_PARILUT_SAME_DEV(LRowMapType, LEntriesType), "par_ilut_numeric: rowmap and entries have different device types.");
  static_assert(KKAMD_PARILUT_SAME_DEV(LRowMapType, LValuesType), "par_ilut_numeric: rowmap and values have different device types.");
  static_assert(std::is_same<ordinal_type, int>::value, "kkamd: ordinals must be int32");
  auto* ih = handle->get_par_ilut_handle();
  if (!ih) throw std::invalid_argument("KokkosSparse::par_ilut_numeric: the given KernelHandle does not have a PAR_ILUT handle associated with it.");
  if (!ih->is_symbolic_complete())
    KokkosKernels::Impl::throw_runtime_exception("KokkosSparse::Experimental::par_ilut_numeric: par_ilut_symbolic "
                                                 "must be called before par_ilut_numeric.");
  if (A_rowmap.extent(0) != 0) {
    if (A_rowmap.size() != L_rowmap.size()) throw std::runtime_error("A rows does not match L rows");
    if (A_rowmap.size() != U_rowmap.size()) throw std::runtime_error("A rows does not match U rows");
  }
  const int64_t nrows = A_rowmap.extent(0) ? (int64_t)A_rowmap.extent(0) - 1 : 0;
  typename KernelHandle::HandleExecSpace space;
  kkamd_stream_t st = reinterpret_cast<kkamd_stream_t>(space.hip_stream());
  Kokkos::View<size_type*, typename ARowMapType::device_type> zero;
  const void* a_rm = A_rowmap.data();
  if (A_rowmap.extent(0) == 0) {
    zero = Kokkos::View<size_type*, typename ARowMapType::device_type>("par_ilut zero row map", 1);
    a_rm = zero.data();
  }
  Kokkos::Profiling::pushRegion("KokkosSparse::par_ilut_numeric[KKAMD]");
  int rc = kkamd_par_ilut_numeric(ih->native(), nrows, a_rm, A_entries.data(), A_values.data(), (void*)L_rowmap.data(), (void*)U_rowmap.data(),
                                  KokkosSparse::Impl::kkamd_offset<size_type>::value, KokkosSparse::Impl::kkamd_scalar<scalar_type>::value, st);
  if (rc == KKAMD_OK) {   // the reference resizes the caller's views every iteration; their final extents are the factors' sizes
    const size_t nl = (size_t)ih->get("nnzL_out"), nu = (size_t)ih->get("nnzU_out");
    Kokkos::resize(L_entries, nl); Kokkos::resize(L_values, nl);
    Kokkos::resize(U_entries, nu); Kokkos::resize(U_values, nu);
    rc = kkamd_par_ilut_copy_factors(ih->native(), L_entries.data(), (void*)L_values.data(), (int64_t)nl, U_entries.data(), (void*)U_values.data(),
                                     (int64_t)nu, st);
    space.fence();
  }
  Kokkos::Profiling::popRegion();
  KokkosSparse::Impl::kkamd_check(rc);
}

#undef KKAMD_PARILUT_SAME
#undef KKAMD_PARILUT_NONCONST
#undef KKAMD_PARILUT_SAME_DEV
#undef KKAMD_PARILUT_EXEC

}}  // namespace KokkosSparse::Experimental
