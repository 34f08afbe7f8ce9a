// KokkosSparse::Experimental::spgemm_jacobi: C = (I - omega D^-1 A) B = B - omega D^-1 (A B), in the place of spgemm_numeric after
// spgemm_symbolic(A, B) on the same handle.  Reference: sparse/src/KokkosSparse_spgemm_jacobi.hpp:26-188 (interface),
// sparse/impl/KokkosSparse_spgemm_jacobi_seq_impl.hpp:65-123 (semantics).  Kept: the argument order, the static_assert texts, the
// std::runtime_error text for a transposed operand, dinv as the reference's rank-2 view with one column (a rank-1 view is taken too).
// Impl::SPGEMM_JACOBI is replaced by one C-ABI call; what it computes, rounding by rounding, is documented at kkamd_spgemm_jacobi in
// include/kkamd.h.  A row of B with a column that row of A * B lacks (a row of A without its diagonal), which the reference writes past
// the row for, is a std::runtime_error here.
#pragma once
#include "KokkosKernels_Handle.hpp"
#include "KokkosSparse_CrsMatrix.hpp"

namespace KokkosSparse {
namespace Experimental {

template <typename KernelHandle, typename alno_row_view_t_, typename alno_nnz_view_t_, typename ascalar_nnz_view_t_,
          typename blno_row_view_t_, typename blno_nnz_view_t_, typename bscalar_nnz_view_t_, typename clno_row_view_t_,
          typename clno_nnz_view_t_, typename cscalar_nnz_view_t_, typename dinv_view_t_>
void spgemm_jacobi(KernelHandle* handle, typename KernelHandle::const_nnz_lno_t m, typename KernelHandle::const_nnz_lno_t n,
                   typename KernelHandle::const_nnz_lno_t k, alno_row_view_t_ row_mapA, alno_nnz_view_t_ entriesA,
                   ascalar_nnz_view_t_ valuesA, bool transposeA, blno_row_view_t_ row_mapB, blno_nnz_view_t_ entriesB,
                   bscalar_nnz_view_t_ valuesB, bool transposeB, clno_row_view_t_ row_mapC, clno_nnz_view_t_& entriesC,
                   cscalar_nnz_view_t_& valuesC, typename cscalar_nnz_view_t_::const_value_type omega, dinv_view_t_ dinv) {
  static_assert(std::is_same<typename clno_row_view_t_::value_type, typename clno_row_view_t_::non_const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: Output matrix rowmap must be non-const.");
  static_assert(std::is_same<typename clno_nnz_view_t_::value_type, typename clno_nnz_view_t_::non_const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: Output matrix entriesView must be "
                "non-const.");
  static_assert(std::is_same<typename cscalar_nnz_view_t_::value_type, typename cscalar_nnz_view_t_::non_const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: Output matrix scalar view must be "
                "non-const.");
  static_assert(std::is_same<typename KernelHandle::const_size_type, typename alno_row_view_t_::const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: Size type of left handside matrix should "
                "be same as kernelHandle sizetype.");
  static_assert(std::is_same<typename KernelHandle::const_size_type, typename blno_row_view_t_::const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: Size type of right handside matrix should "
                "be same as kernelHandle sizetype.");
  static_assert(std::is_same<typename KernelHandle::const_size_type, typename clno_row_view_t_::const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: Size type of output matrix should be same "
                "as kernelHandle sizetype.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_lno_t, typename alno_nnz_view_t_::const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: lno type of left handside matrix should be "
                "same as kernelHandle lno_t.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_lno_t, typename blno_nnz_view_t_::const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: lno type of right handside matrix should "
                "be same as kernelHandle lno_t.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_lno_t, typename clno_nnz_view_t_::const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: lno type of output matrix should be same "
                "as kernelHandle lno_t.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_scalar_t, typename ascalar_nnz_view_t_::const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: scalar type of left handside matrix should "
                "be same as kernelHandle scalar.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_scalar_t, typename bscalar_nnz_view_t_::const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: scalar type of right handside matrix "
                "should be same as kernelHandle scalar.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_scalar_t, typename cscalar_nnz_view_t_::const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: scalar type of output matrix should be "
                "same as kernelHandle scalar.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_scalar_t, typename dinv_view_t_::const_value_type>::value,
                "KokkosSparse::spgemm_jacobi: scalar type of dinv should be same as kernelHandle scalar.");
  if (transposeA || transposeB) {
    throw std::runtime_error(
        "spgemm-jacobi does not support transposed multiply. "
        "If you need this case please let kokkos-kernels developers know.\n");
  }
  auto* sh = handle->get_spgemm_handle();
  if (!sh) throw std::invalid_argument("KokkosSparse::spgemm_jacobi: the given KernelHandle does not have an SpGEMM handle associated with it.");
  if ((size_t)dinv.extent(0) != (size_t)m || dinv.extent(1) != 1 || ((size_t)m > 1 && dinv.stride(0) != 1))
    throw std::runtime_error("KokkosSparse::spgemm_jacobi: dinv must hold m contiguous values (rank 1, or rank 2 with one column)");
  Kokkos::Profiling::pushRegion("KokkosSparse::spgemm_jacobi[KKAMD]");
  Impl::kkamd_check(kkamd_spgemm_jacobi(sh->native(), m, n, k, row_mapA.data(), entriesA.data(), valuesA.data(), row_mapB.data(), entriesB.data(),
                                        valuesB.data(), row_mapC.data(), (int32_t*)entriesC.data(), (void*)valuesC.data(), (double)omega, dinv.data(),
                                        Impl::kkamd_offset<typename alno_row_view_t_::non_const_value_type>::value,
                                        Impl::kkamd_scalar<typename ascalar_nnz_view_t_::non_const_value_type>::value, nullptr));
  Kokkos::Profiling::popRegion();
}

}  // namespace Experimental
}  // namespace KokkosSparse
