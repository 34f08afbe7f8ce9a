// KokkosSparse::gauss_seidel_symbolic / gauss_seidel_numeric / symmetric_gauss_seidel_apply / forward_sweep_gauss_seidel_apply /
// backward_sweep_gauss_seidel_apply -- reference: sparse/src/KokkosSparse_gauss_seidel.hpp:45-134 (symbolic, with and without an
// execution space), :173-400 (numeric, with and without given_inverse_diagonal), :462-640 (symmetric apply), :704-884 (forward),
// :949-1129 (backward), :1163-1410 (the KokkosSparse::Experimental:: names).  Kept: argument order and defaults, the format template
// parameter (CRS only), rank-1 and rank-2 x / y in LayoutLeft or LayoutRight, the column-count check and its text, "the handle must
// carry a Gauss-Seidel sub-handle".  Impl::GAUSS_SEIDEL_SYMBOLIC / _NUMERIC / _APPLY are replaced by the three C-ABI calls, on the
// execution space's stream.  Not here: the block_* entry points (BSR).
#pragma once
#include "KokkosKernels_Handle.hpp"

namespace KokkosSparse {

namespace Impl {
template <class KernelHandle>
auto* kkamd_gs_sub_handle(KernelHandle* handle, const char* who) {
  auto* gh = handle->get_gs_handle();
  if (!gh) throw std::invalid_argument(std::string("KokkosSparse::") + who + ": the given KernelHandle does not have a Gauss-Seidel handle associated with it.");
  return gh;
}

template <class ExecutionSpace, class KernelHandle, class lno_row_view_t_, class lno_nnz_view_t_, class scalar_nnz_view_t_, class x_scalar_view_t,
          class y_scalar_view_t>
void kkamd_gs_apply_views(const char* who, int direction, const ExecutionSpace& space, KernelHandle* handle, int64_t num_rows, int64_t num_cols,
                          lno_row_view_t_ row_map, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values, x_scalar_view_t x, y_scalar_view_t y,
                          bool init_zero_x_vector, bool update_y_vector, typename KernelHandle::nnz_scalar_t omega, int numIter) {
  typedef typename KernelHandle::size_type size_type;
  typedef typename KernelHandle::nnz_scalar_t scalar_type;
  static_assert(std::is_same<typename KernelHandle::const_size_type, typename lno_row_view_t_::const_value_type>::value,
                "KokkosSparse::gauss_seidel_apply: Size type of the matrix should be same as kernelHandle sizetype.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_lno_t, typename lno_nnz_view_t_::const_value_type>::value,
                "KokkosSparse::gauss_seidel_apply: lno type of the matrix should be same as kernelHandle lno_t.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_scalar_t, typename scalar_nnz_view_t_::const_value_type>::value,
                "KokkosSparse::gauss_seidel_apply: scalar type of the matrix should be same as kernelHandle scalar_t.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_scalar_t, typename y_scalar_view_t::const_value_type>::value,
                "KokkosSparse::gauss_seidel_apply: scalar type of the y-vector should be same as kernelHandle scalar_t.");
  static_assert(std::is_same<typename KernelHandle::nnz_scalar_t, typename x_scalar_view_t::value_type>::value,
                "KokkosSparse::gauss_seidel_apply: scalar type of the x-vector should be same as kernelHandle non-const scalar_t.");
  static_assert((int)x_scalar_view_t::rank() == (int)y_scalar_view_t::rank() && (x_scalar_view_t::rank() == 1 || x_scalar_view_t::rank() == 2),
                "KokkosSparse::gauss_seidel_apply: x and y must both have rank 1 or both rank 2.");
  static_assert(std::is_same<typename KernelHandle::nnz_lno_t, int>::value, "kkamd: ordinals must be int32");
  if (x.extent(1) != y.extent(1))
    throw std::runtime_error(std::string("KokkosSparse::") + who + ": X has " + std::to_string(x.extent(1)) + "columns, Y has " +
                             std::to_string(y.extent(1)) + " columns.");
  if ((int64_t)x.extent(0) < num_cols || (int64_t)y.extent(0) < num_rows)
    throw std::runtime_error(std::string("KokkosSparse::") + who + ": x needs num_cols rows and y num_rows rows");
  auto* gh = kkamd_gs_sub_handle(handle, who);
  Kokkos::Profiling::pushRegion("KokkosSparse::gauss_seidel_apply[KKAMD]");
  const int rc = kkamd_gs_apply(gh->native(), num_rows, num_cols, row_map.data(), entries.data(), values.data(), (void*)x.data(), (int64_t)x.stride(0),
                                (int64_t)x.stride(1), y.data(), (int64_t)y.stride(0), (int64_t)y.stride(1), (int64_t)x.extent(1), init_zero_x_vector ? 1 : 0,
                                update_y_vector ? 1 : 0, (double)omega, numIter, direction, kkamd_offset<size_type>::value, kkamd_scalar<scalar_type>::value,
                                reinterpret_cast<kkamd_stream_t>(space.hip_stream()));
  Kokkos::Profiling::popRegion();
  kkamd_check(rc);
}
}  // namespace Impl

template <typename ExecutionSpace, typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_>
void gauss_seidel_symbolic(const ExecutionSpace& space, KernelHandle* handle, typename KernelHandle::const_nnz_lno_t num_rows,
                           typename KernelHandle::const_nnz_lno_t num_cols, lno_row_view_t_ row_map, lno_nnz_view_t_ entries,
                           bool is_graph_symmetric = true) {
  static_assert(std::is_same<typename KernelHandle::const_size_type, typename lno_row_view_t_::const_value_type>::value,
                "KokkosSparse::gauss_seidel_symbolic: Size type of the matrix should be same as kernelHandle sizetype.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_lno_t, typename lno_nnz_view_t_::const_value_type>::value,
                "KokkosSparse::gauss_seidel_symbolic: lno type of the matrix should be same as kernelHandle lno_t.");
  static_assert(std::is_same<typename KernelHandle::nnz_lno_t, int>::value, "kkamd: ordinals must be int32");
  auto* gh = Impl::kkamd_gs_sub_handle(handle, "gauss_seidel_symbolic");
  if ((int64_t)row_map.extent(0) != (int64_t)num_rows + 1 && !(num_rows == 0 && row_map.extent(0) == 0))
    throw std::runtime_error("KokkosSparse::gauss_seidel_symbolic: row_map must have num_rows + 1 entries");
  Kokkos::Profiling::pushRegion("KokkosSparse::gauss_seidel_symbolic[KKAMD]");
  const int rc = kkamd_gs_symbolic(gh->native(), num_rows, num_cols, row_map.data(), entries.data(), Impl::kkamd_offset<typename KernelHandle::size_type>::value,
                                   is_graph_symmetric ? 1 : 0, nullptr, reinterpret_cast<kkamd_stream_t>(space.hip_stream()));
  Kokkos::Profiling::popRegion();
  Impl::kkamd_check(rc);
}

template <typename KernelHandle, typename lno_row_view_t_, typename lno_nnz_view_t_>
void gauss_seidel_symbolic(KernelHandle* handle, typename KernelHandle::const_nnz_lno_t num_rows, typename KernelHandle::const_nnz_lno_t num_cols,
                           lno_row_view_t_ row_map, lno_nnz_view_t_ entries, bool is_graph_symmetric = true) {
  auto my_exec_space = typename KernelHandle::HandleExecSpace();
  gauss_seidel_symbolic(my_exec_space, handle, num_rows, num_cols, row_map, entries, is_graph_symmetric);
}

// with the caller's inverse diagonal (:296-400)
template <class ExecutionSpace, KokkosSparse::SparseMatrixFormat format = KokkosSparse::SparseMatrixFormat::CRS, typename KernelHandle,
          typename lno_row_view_t_, typename lno_nnz_view_t_, typename scalar_nnz_view_t_>
void gauss_seidel_numeric(const ExecutionSpace& space, KernelHandle* handle, typename KernelHandle::const_nnz_lno_t num_rows,
                          typename KernelHandle::const_nnz_lno_t num_cols, lno_row_view_t_ row_map, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values,
                          scalar_nnz_view_t_ given_inverse_diagonal, bool /*is_graph_symmetric*/ = true) {
  static_assert(format == KokkosSparse::SparseMatrixFormat::CRS, "kkamd: block (BSR) Gauss-Seidel is not implemented");
  static_assert(std::is_same<typename KernelHandle::const_size_type, typename lno_row_view_t_::const_value_type>::value,
                "KokkosSparse::gauss_seidel_numeric: Size type of the matrix should be same as kernelHandle sizetype.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_lno_t, typename lno_nnz_view_t_::const_value_type>::value,
                "KokkosSparse::gauss_seidel_numeric: lno type of the matrix should be same as kernelHandle lno_t.");
  static_assert(std::is_same<typename KernelHandle::const_nnz_scalar_t, typename scalar_nnz_view_t_::const_value_type>::value,
                "KokkosSparse::gauss_seidel_numeric: scalar type of the matrix should be same as kernelHandle scalar_t.");
  auto* gh = Impl::kkamd_gs_sub_handle(handle, "gauss_seidel_numeric");
  if (given_inverse_diagonal.data() && (int64_t)given_inverse_diagonal.extent(0) < (int64_t)num_rows)
    throw std::runtime_error("KokkosSparse::gauss_seidel_numeric: given_inverse_diagonal must have num_rows entries");
  Kokkos::Profiling::pushRegion("KokkosSparse::gauss_seidel_numeric[KKAMD]");
  const int rc = kkamd_gs_numeric(gh->native(), num_rows, num_cols, row_map.data(), entries.data(), values.data(), given_inverse_diagonal.data(),
                                  Impl::kkamd_offset<typename KernelHandle::size_type>::value, Impl::kkamd_scalar<typename KernelHandle::nnz_scalar_t>::value,
                                  reinterpret_cast<kkamd_stream_t>(space.hip_stream()));
  Kokkos::Profiling::popRegion();
  Impl::kkamd_check(rc);
}

template <class ExecutionSpace, KokkosSparse::SparseMatrixFormat format = KokkosSparse::SparseMatrixFormat::CRS, typename KernelHandle,
          typename lno_row_view_t_, typename lno_nnz_view_t_, typename scalar_nnz_view_t_>
void gauss_seidel_numeric(const ExecutionSpace& space, KernelHandle* handle, typename KernelHandle::const_nnz_lno_t num_rows,
                          typename KernelHandle::const_nnz_lno_t num_cols, lno_row_view_t_ row_map, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values,
                          bool is_graph_symmetric = true) {
  gauss_seidel_numeric<ExecutionSpace, format>(space, handle, num_rows, num_cols, row_map, entries, values, scalar_nnz_view_t_(), is_graph_symmetric);
}

template <KokkosSparse::SparseMatrixFormat format = KokkosSparse::SparseMatrixFormat::CRS, typename KernelHandle, typename lno_row_view_t_,
          typename lno_nnz_view_t_, typename scalar_nnz_view_t_>
void gauss_seidel_numeric(KernelHandle* handle, typename KernelHandle::const_nnz_lno_t num_rows, typename KernelHandle::const_nnz_lno_t num_cols,
                          lno_row_view_t_ row_map, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values, bool is_graph_symmetric = true) {
  auto my_exec_space = typename KernelHandle::HandleExecSpace();
  gauss_seidel_numeric<typename KernelHandle::HandleExecSpace, format>(my_exec_space, handle, num_rows, num_cols, row_map, entries, values, is_graph_symmetric);
}

template <KokkosSparse::SparseMatrixFormat format = KokkosSparse::SparseMatrixFormat::CRS, typename KernelHandle, typename lno_row_view_t_,
          typename lno_nnz_view_t_, typename scalar_nnz_view_t_>
void gauss_seidel_numeric(KernelHandle* handle, typename KernelHandle::const_nnz_lno_t num_rows, typename KernelHandle::const_nnz_lno_t num_cols,
                          lno_row_view_t_ row_map, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values, scalar_nnz_view_t_ given_inverse_diagonal,
                          bool is_graph_symmetric = true) {
  auto my_exec_space = typename KernelHandle::HandleExecSpace();
  gauss_seidel_numeric<typename KernelHandle::HandleExecSpace, format>(my_exec_space, handle, num_rows, num_cols, row_map, entries, values,
                                                                       given_inverse_diagonal, is_graph_symmetric);
}

// the three apply functions, each with and without an execution space instance
#define KKAMD_GS_APPLY(NAME, DIRECTION)                                                                                                            \
  template <class ExecutionSpace, KokkosSparse::SparseMatrixFormat format = KokkosSparse::SparseMatrixFormat::CRS, typename KernelHandle,          \
            typename lno_row_view_t_, typename lno_nnz_view_t_, typename scalar_nnz_view_t_, typename x_scalar_view_t, typename y_scalar_view_t>  \
  void NAME(const ExecutionSpace& space, KernelHandle* handle, typename KernelHandle::const_nnz_lno_t num_rows,                                    \
            typename KernelHandle::const_nnz_lno_t num_cols, lno_row_view_t_ row_map, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values,          \
            x_scalar_view_t x_lhs_output_vec, y_scalar_view_t y_rhs_input_vec, bool init_zero_x_vector, bool update_y_vector,                      \
            typename KernelHandle::nnz_scalar_t omega, int numIter) {                                                                              \
    static_assert(format == KokkosSparse::SparseMatrixFormat::CRS, "kkamd: block (BSR) Gauss-Seidel is not implemented");                          \
    Impl::kkamd_gs_apply_views(#NAME, DIRECTION, space, handle, num_rows, num_cols, row_map, entries, values, x_lhs_output_vec, y_rhs_input_vec,    \
                               init_zero_x_vector, update_y_vector, omega, numIter);                                                               \
  }                                                                                                                                                \
  template <KokkosSparse::SparseMatrixFormat format = KokkosSparse::SparseMatrixFormat::CRS, typename KernelHandle, typename lno_row_view_t_,      \
            typename lno_nnz_view_t_, typename scalar_nnz_view_t_, typename x_scalar_view_t, typename y_scalar_view_t>                            \
  void NAME(KernelHandle* handle, typename KernelHandle::const_nnz_lno_t num_rows, typename KernelHandle::const_nnz_lno_t num_cols,                \
            lno_row_view_t_ row_map, lno_nnz_view_t_ entries, scalar_nnz_view_t_ values, x_scalar_view_t x_lhs_output_vec,                         \
            y_scalar_view_t y_rhs_input_vec, bool init_zero_x_vector, bool update_y_vector, typename KernelHandle::nnz_scalar_t omega,            \
            int numIter) {                                                                                                                         \
    auto my_exec_space = typename KernelHandle::HandleExecSpace();                                                                                 \
    NAME<typename KernelHandle::HandleExecSpace, format>(my_exec_space, handle, num_rows, num_cols, row_map, entries, values, x_lhs_output_vec,     \
                                                         y_rhs_input_vec, init_zero_x_vector, update_y_vector, omega, numIter);                    \
  }
KKAMD_GS_APPLY(symmetric_gauss_seidel_apply, KKAMD_GS_SYMMETRIC)
KKAMD_GS_APPLY(forward_sweep_gauss_seidel_apply, KKAMD_GS_FORWARD)
KKAMD_GS_APPLY(backward_sweep_gauss_seidel_apply, KKAMD_GS_BACKWARD)
#undef KKAMD_GS_APPLY

// the reference keeps forwarding functions of the same names in KokkosSparse::Experimental (:1163-1410)
namespace Experimental {
using KokkosSparse::gauss_seidel_symbolic;
using KokkosSparse::gauss_seidel_numeric;
using KokkosSparse::symmetric_gauss_seidel_apply;
using KokkosSparse::forward_sweep_gauss_seidel_apply;
using KokkosSparse::backward_sweep_gauss_seidel_apply;
}  // namespace Experimental

}  // namespace KokkosSparse
