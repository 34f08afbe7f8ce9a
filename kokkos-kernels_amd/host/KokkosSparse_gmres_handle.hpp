// KokkosSparse::Experimental::GMRESHandle -- reference: sparse/src/KokkosSparse_gmres_handle.hpp:38-181 (Ortho :76-79, Flag :84-89,
// constructor and reset_handle :107-130, setters :136-163, results :165-180).  m, tol, max_restart, ortho, verbose and the results live
// in the library's kkamd_gmres_handle together with its workspace (the basis, the work vectors, the partial slabs, the SpMV plan);
// this class forwards to it.  The reference asserts that a solve has run in get_num_iters / get_end_rel_res; so does this one.
#pragma once
#include <cassert>
#include <string>
#include <vector>
#include "Kokkos_Shim.hpp"
#include "kkamd_status.hpp"

namespace KokkosSparse { namespace Experimental {

template <class size_type_, class lno_t_, class scalar_t_, class ExecutionSpace, class TemporaryMemorySpace, class PersistentMemorySpace>
class GMRESHandle {
 public:
  using HandleExecSpace             = ExecutionSpace;
  using HandleTempMemorySpace       = TemporaryMemorySpace;
  using HandlePersistentMemorySpace = PersistentMemorySpace;
  using execution_space             = ExecutionSpace;
  using memory_space                = HandlePersistentMemorySpace;
  using size_type                   = std::remove_const_t<size_type_>;
  using nnz_lno_t                   = std::remove_const_t<lno_t_>;
  using nnz_scalar_t                = std::remove_const_t<scalar_t_>;
  using float_t                     = nnz_scalar_t;      // ArithTraits<nnz_scalar_t>::mag_type of a real scalar

  enum Ortho { CGS2, MGS };
  enum Flag { Conv, NoConv, LOA, NotRun };

  GMRESHandle(const size_type m_ = 50, const float_t tol_ = 1e-8, const size_type max_restart_ = 50) {
    const int rc = kkamd_gmres_create(&h_, (int64_t)m_, (double)tol_, (int64_t)max_restart_);
    if (rc == KKAMD_ERR_INVALID_ARG) throw std::invalid_argument(kkamd_last_error());   // "gmres: Please choose restart size m greater than zero."
    KokkosSparse::Impl::kkamd_check(rc);
  }
  ~GMRESHandle() { if (h_) kkamd_gmres_destroy(h_); }
  GMRESHandle(const GMRESHandle&)            = delete;
  GMRESHandle& operator=(const GMRESHandle&) = delete;

  void reset_handle(const size_type m_ = 50, const float_t tol_ = 1e-8, const size_type max_restart_ = 50) {
    KokkosSparse::Impl::kkamd_check(kkamd_gmres_reset(h_, (int64_t)m_, (double)tol_, (int64_t)max_restart_));
  }
  kkamd_gmres_handle_t* native() const { return h_; }
  size_type get_m() const { return (size_type)get("m"); }
  void set_m(const size_type m_) { set("m", (int64_t)m_); }
  size_type get_max_restart() const { return (size_type)get("max_restart"); }
  void set_max_restart(const size_type r) { set("max_restart", (int64_t)r); }
  float_t get_tol() const { return (float_t)get_real("tol"); }
  void set_tol(const float_t tol_) { KokkosSparse::Impl::kkamd_check(kkamd_gmres_set_tol(h_, (double)tol_)); }
  Ortho get_ortho() const { return (Ortho)get("ortho"); }
  void set_ortho(const Ortho o) { set("ortho", (int64_t)o); }
  bool get_verbose() const { return get("verbose") != 0; }
  void set_verbose(const bool v) { set("verbose", v ? 1 : 0); }
  int get_num_iters() const { assert(get_conv_flag_val() != NotRun); return (int)get("num_iters"); }
  float_t get_end_rel_res() const { assert(get_conv_flag_val() != NotRun); return (float_t)get_real("end_rel_res"); }
  Flag get_conv_flag_val() const { return (Flag)get("conv_flag"); }
  // the library's knobs and counters (kkamd_gmres_set / _get / _get_real) and its host arrays (kkamd_gmres_export)
  void set(const char* key, int64_t value) { KokkosSparse::Impl::kkamd_check(kkamd_gmres_set(h_, key, value)); }
  int64_t get(const char* key) const { int64_t v = 0; KokkosSparse::Impl::kkamd_check(kkamd_gmres_get(h_, key, &v)); return v; }
  double get_real(const char* key) const { double v = 0; KokkosSparse::Impl::kkamd_check(kkamd_gmres_get_real(h_, key, &v)); return v; }
  std::vector<double> export_host(const char* what) const {
    const std::string w(what);
    const int64_t m = get("m");
    const int64_t count = w == "hessenberg" ? (m + 1) * m : w == "basis" ? get("num_rows") * (m + 1) : get(("num_" + w).c_str());
    std::vector<double> out((size_t)count);
    KokkosSparse::Impl::kkamd_check(kkamd_gmres_export(h_, what, out.data(), count));
    return out;
  }
 private:
  kkamd_gmres_handle_t* h_ = nullptr;
};

}}  // namespace KokkosSparse::Experimental
