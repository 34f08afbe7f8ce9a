// KokkosSparse::Experimental::gmres -- reference: sparse/src/KokkosSparse_gmres.hpp:58-158.  Kept: the signature, the static asserts
// (scalar, ordinal and size types of A, B, X against the handle's; A a CrsMatrix; rank-1 views; a non-const X), the dimension check and
// its text (:110-116).  Impl::GMRES<...>::gmres is replaced by kkamd_gmres_solve on the handle's execution space's stream; a lucky
// breakdown and a NaN residual come back as std::runtime_error with the reference's messages.  Not here: BSR matrices.
#pragma once
#include <sstream>
#include "KokkosKernels_Handle.hpp"
#include "KokkosSparse_Preconditioner.hpp"
#include "KokkosSparse_spmv.hpp"

namespace KokkosSparse { namespace Experimental {

#define KOKKOSKERNELS_GMRES_SAME_TYPE(A, B) std::is_same<std::remove_const_t<A>, std::remove_const_t<B>>::value

template <typename KernelHandle, typename AMatrix, typename BType, typename XType>
void gmres(KernelHandle* handle, AMatrix& A, BType& B, XType& X, Preconditioner<AMatrix>* precond = nullptr) {
  using scalar_type  = typename KernelHandle::nnz_scalar_t;
  using size_type    = typename KernelHandle::size_type;
  using ordinal_type = typename KernelHandle::nnz_lno_t;
  static_assert(KOKKOSKERNELS_GMRES_SAME_TYPE(typename BType::value_type, scalar_type),
                "gmres: B scalar type must match KernelHandle entry type (aka nnz_scalar_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_GMRES_SAME_TYPE(typename XType::value_type, scalar_type),
                "gmres: X scalar type must match KernelHandle entry type (aka nnz_scalar_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_GMRES_SAME_TYPE(typename AMatrix::value_type, scalar_type),
                "gmres: A scalar type must match KernelHandle entry type (aka nnz_scalar_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_GMRES_SAME_TYPE(typename AMatrix::ordinal_type, ordinal_type),
                "gmres: A ordinal type must match KernelHandle entry type (aka nnz_lno_t, and const doesn't matter)");
  static_assert(KOKKOSKERNELS_GMRES_SAME_TYPE(typename AMatrix::size_type, size_type),
                "gmres: A size type must match KernelHandle entry type (aka size_type, and const doesn't matter)");
  static_assert(KokkosSparse::is_crs_matrix<AMatrix>::value, "gmres: A is not a CRS matrix (kkamd: BSR is not implemented).");
  static_assert(BType::rank() == 1, "gmres: B must have rank 1");
  static_assert(XType::rank() == 1, "gmres: X must have rank 1");
  static_assert(std::is_same<typename XType::value_type, typename XType::non_const_value_type>::value, "gmres: The output X must be nonconst.");

  if ((X.extent(0) != B.extent(0)) || (static_cast<size_t>(A.numCols()) != static_cast<size_t>(X.extent(0))) ||
      (static_cast<size_t>(A.numRows()) != static_cast<size_t>(B.extent(0)))) {
    std::ostringstream os;
    os << "KokkosSparse::gmres: Dimensions do not match: "
       << ", A: " << A.numRows() << " x " << A.numCols() << ", x: " << X.extent(0) << ", b: " << B.extent(0);
    throw std::runtime_error(os.str());
  }
  auto* gh = handle->get_gmres_handle();
  if (!gh) throw std::invalid_argument("KokkosSparse::gmres: the given KernelHandle does not have a GMRES handle associated with it.");
  kkamd_crs_t d = KokkosSparse::Impl::make_crs_desc(A);
  auto space    = typename KernelHandle::HandleExecSpace();
  Kokkos::Profiling::pushRegion("KokkosSparse::gmres[KKAMD]");
  const int rc = kkamd_gmres_solve(gh->native(), &d, B.data(), X.data(), precond ? precond->native((int64_t)A.numRows()) : nullptr,
                                   KokkosSparse::Impl::kkamd_scalar<scalar_type>::value, reinterpret_cast<kkamd_stream_t>(space.hip_stream()));
  Kokkos::Profiling::popRegion();
  KokkosSparse::Impl::kkamd_check(rc);
}

#undef KOKKOSKERNELS_GMRES_SAME_TYPE

}}  // namespace KokkosSparse::Experimental
