// KokkosSparse::Experimental::LUPrec<CRS, KernelHandle> -- reference: sparse/src/KokkosSparse_LUPrec.hpp:43-119: Y = alpha U^-1 L^-1 X +
// beta Y by two triangular solves.  The library's LU kind owns the two sptrsv handles and analyses ONCE, at construction; the reference
// calls sptrsv_symbolic again at every apply (:94-98).  L carries its unit diagonal and U its diagonal, as spiluk_numeric leaves them.
#pragma once
#include "KokkosSparse_Preconditioner.hpp"
#include "KokkosSparse_spmv.hpp"

namespace KokkosSparse { namespace Experimental {

template <class CRS, class KernelHandle>
class LUPrec : public Preconditioner<CRS> {
 public:
  using ScalarType = typename Preconditioner<CRS>::ScalarType;
  using DEVICE     = typename Preconditioner<CRS>::DEVICE;
  using size_type  = typename CRS::size_type;

  template <class CRSArg>
  LUPrec(const CRSArg& L, const CRSArg& U, const size_type block_size = 0) : L_(L), U_(U) {
    if (block_size != 0) throw std::runtime_error("LUPrec (kkamd): block (BSR) factors are not implemented");
    if (L.numRows() != U.numRows()) throw std::runtime_error("LUPrec: L.numRows() != U.numRows()");
    kkamd_crs_t dl = KokkosSparse::Impl::make_crs_desc(L_), du = KokkosSparse::Impl::make_crs_desc(U_);
    KokkosSparse::Impl::kkamd_check(kkamd_precond_create_lu(&this->p_, &dl, &du, nullptr));
  }
  virtual ~LUPrec() {}

  virtual void apply(const Kokkos::View<const ScalarType*, DEVICE>& X, const Kokkos::View<ScalarType*, DEVICE>& Y, const char transM[] = "N",
                     ScalarType alpha = ScalarType(1), ScalarType beta = ScalarType(0)) const {
    if (transM[0] != 'N') throw std::runtime_error("LUPrec::apply only supports 'N' for transM");
    KokkosSparse::Impl::kkamd_check(kkamd_precond_apply(this->p_, X.data(), Y.data(), (double)alpha, (double)beta,
                                                        KokkosSparse::Impl::kkamd_scalar<ScalarType>::value, nullptr));
  }
  bool hasTransposeApply() const { return true; }
 private:
  CRS L_, U_;
};

}}  // namespace KokkosSparse::Experimental
