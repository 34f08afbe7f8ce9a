// KokkosSparse::Experimental::Preconditioner<CRS> -- reference: sparse/src/KokkosSparse_Preconditioner.hpp:55-112: the interface GMRES
// applies, Y = beta * Y + alpha * M * X.  Every preconditioner owns a kkamd_precond_t that the solver calls: MatrixPrec and LUPrec create
// the library's own kinds; a user's subclass gets the callback kind, whose function wraps the raw device pointers into unmanaged views
// and calls the virtual apply -- so a Gauss-Seidel smoother or any foreign operator written against this interface works under gmres.
#pragma once
#include "KokkosSparse_CrsMatrix.hpp"
#include "kkamd_status.hpp"

namespace KokkosSparse { namespace Experimental {

template <class CRS>
class Preconditioner {
 public:
  using ScalarType = std::remove_const_t<typename CRS::value_type>;
  using EXSP       = typename CRS::execution_space;
  using MEMSP      = typename CRS::memory_space;
  using DEVICE     = Kokkos::Device<EXSP, MEMSP>;

  Preconditioner() {}
  virtual ~Preconditioner() { if (p_) kkamd_precond_destroy(p_); }
  Preconditioner(const Preconditioner&)            = delete;
  Preconditioner& operator=(const Preconditioner&) = delete;

  virtual void apply(const Kokkos::View<const ScalarType*, DEVICE>& X, const Kokkos::View<ScalarType*, DEVICE>& Y, const char transM[] = "N",
                     ScalarType alpha = ScalarType(1), ScalarType beta = ScalarType(0)) const = 0;
  virtual void setParameters() {}
  virtual void initialize() {}
  virtual bool isInitialized() const { return true; }
  virtual void compute() {}
  virtual bool isComputed() const { return true; }
  virtual bool hasTransposeApply() const { return false; }

  // what gmres hands to the library: the subclass's own kind, or on first use the callback kind bound to the virtual apply.
  // n: the length of the vectors (the callback receives raw pointers).
  kkamd_precond_t* native(int64_t n) {
    n_ = n;
    if (!p_) KokkosSparse::Impl::kkamd_check(kkamd_precond_create_callback(&p_, &Preconditioner::trampoline, this));
    return p_;
  }

 protected:
  kkamd_precond_t* p_ = nullptr;

 private:
  int64_t n_ = 0;
  static int trampoline(void* ctx, const void* d_x, void* d_y, double alpha, double beta, int /*value_type*/, kkamd_stream_t /*stream*/) {
    auto* self = static_cast<Preconditioner*>(ctx);
    try {
      Kokkos::View<const ScalarType*, DEVICE> X(static_cast<const ScalarType*>(d_x), (size_t)self->n_);
      Kokkos::View<ScalarType*, DEVICE> Y(static_cast<ScalarType*>(d_y), (size_t)self->n_);
      self->apply(X, Y, "N", (ScalarType)alpha, (ScalarType)beta);
    } catch (...) {
      return KKAMD_ERR_INVALID_ARG;
    }
    return KKAMD_OK;
  }
};

}}  // namespace KokkosSparse::Experimental
