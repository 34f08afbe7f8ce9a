// KokkosSparse::Experimental::MatrixPrec<CRS> -- reference: sparse/src/KokkosSparse_MatrixPrec.hpp:45-101: the preconditioner is a
// matrix, apply is spmv(transM, alpha, M, X, beta, Y).  The library's matrix kind keeps an SpMV plan of its own; only "N" is supported.
#pragma once
#include "KokkosSparse_Preconditioner.hpp"
#include "KokkosSparse_spmv.hpp"

namespace KokkosSparse { namespace Experimental {

template <class CRS>
class MatrixPrec : public Preconditioner<CRS> {
 public:
  using ScalarType = typename Preconditioner<CRS>::ScalarType;
  using DEVICE     = typename Preconditioner<CRS>::DEVICE;

  template <class CRSArg>
  MatrixPrec(const CRSArg& mat) : A_(mat) {
    kkamd_crs_t d = KokkosSparse::Impl::make_crs_desc(A_);
    KokkosSparse::Impl::kkamd_check(kkamd_precond_create_matrix(&this->p_, &d, nullptr));
  }
  virtual ~MatrixPrec() {}

  virtual void apply(const Kokkos::View<const ScalarType*, DEVICE>& X, const Kokkos::View<ScalarType*, DEVICE>& Y, const char transM[] = "N",
                     ScalarType alpha = ScalarType(1), ScalarType beta = ScalarType(0)) const {
    if (transM[0] != 'N' && transM[0] != 'n') throw std::runtime_error("MatrixPrec::apply (kkamd) only supports 'N' for transM");
    KokkosSparse::Impl::kkamd_check(kkamd_precond_apply(this->p_, X.data(), Y.data(), (double)alpha, (double)beta,
                                                        KokkosSparse::Impl::kkamd_scalar<ScalarType>::value, nullptr));
  }
 private:
  CRS A_;
};

}}  // namespace KokkosSparse::Experimental
