// PAR_ILUTHandle -- reference: sparse/src/KokkosSparse_par_ilut_handle.hpp:55-200.
// The five user inputs, nrows / nnzL / nnzU of the symbolic phase, the results of the numeric phase and every workspace live in the library's
// kkamd_par_ilut_handle; this class forwards to it.  Kept from the reference: the constructor's arguments (the defaults are
// KokkosKernelsHandle::create_par_ilut_handle's), get_nrows / get_nnzL / get_nnzU, is_symbolic_complete / reset_symbolic_complete, the
// getters and setters of max_iter, residual_norm_delta_stop, fill_in_limit, async_update (recorded, without effect: the reference's numeric
// phase forces it off) and verbose, get_num_iters / get_end_rel_res (-1 before a numeric call), set_team_size / set_vector_size (hints:
// recorded and without effect, like the KernelHandle's; the lanes per row, which the factors' bits depend on, are set only through
// set("lanes_per_row", ...)).  Not here: get_default_team_policy, set_nrows / set_nnzL / set_nnzU
// / set_stats, which only the reference's implementation calls.
#pragma once
#include <string>
#include "Kokkos_Shim.hpp"
#include "kkamd_status.hpp"

namespace KokkosSparse { namespace Experimental {

template <class size_type_, class lno_t_, class scalar_t_, class ExecutionSpace, class TemporaryMemorySpace, class PersistentMemorySpace>
class PAR_ILUTHandle {
 public:
  using HandleExecSpace             = ExecutionSpace;
  using HandleTempMemorySpace       = TemporaryMemorySpace;
  using HandlePersistentMemorySpace = PersistentMemorySpace;
  using execution_space             = ExecutionSpace;
  using memory_space                = HandlePersistentMemorySpace;
  using size_type                   = std::remove_const_t<size_type_>;
  using const_size_type             = const size_type;
  using nnz_lno_t                   = std::remove_const_t<lno_t_>;
  using const_nnz_lno_t             = const nnz_lno_t;
  using nnz_scalar_t                = std::remove_const_t<scalar_t_>;
  using const_nnz_scalar_t          = const nnz_scalar_t;
  using float_t                     = nnz_scalar_t;      // ArithTraits<nnz_scalar_t>::mag_type of a real scalar

  PAR_ILUTHandle(const size_type max_iter_, const float_t residual_norm_delta_stop_, const float_t fill_in_limit_, const bool async_update_,
                 const bool verbose_) {
    KokkosSparse::Impl::kkamd_check(kkamd_par_ilut_create(&h_, (int64_t)max_iter_, (double)residual_norm_delta_stop_, (double)fill_in_limit_,
                                                          async_update_ ? 1 : 0, verbose_ ? 1 : 0));
  }
  ~PAR_ILUTHandle() { if (h_) kkamd_par_ilut_destroy(h_); }
  PAR_ILUTHandle(const PAR_ILUTHandle&)            = delete;
  PAR_ILUTHandle& operator=(const PAR_ILUTHandle&) = delete;

  kkamd_par_ilut_handle_t* native() const { return h_; }
  size_type get_nrows() const { return (size_type)get("num_rows"); }
  size_type get_nnzL() const { return (size_type)get("nnzL"); }
  size_type get_nnzU() const { return (size_type)get("nnzU"); }
  bool is_symbolic_complete() const { return !reset_ && get("symbolic_complete") != 0; }
  void set_symbolic_complete() { reset_ = false; }
  void reset_symbolic_complete() { reset_ = true; }
  void set_team_size(const int ts) { team_size = ts; }
  int get_team_size() const { return team_size; }
  void set_vector_size(const int vs) { vector_size = vs; }
  int get_vector_size() const { return vector_size; }
  void set_max_iter(const size_type v) { set("max_iter", (double)v); }
  int get_max_iter() const { return (int)get("max_iter"); }
  void set_residual_norm_delta_stop(const float_t v) { set("residual_norm_delta_stop", (double)v); }
  float_t get_residual_norm_delta_stop() const { return (float_t)get_real("residual_norm_delta_stop"); }
  void set_fill_in_limit(const float_t v) { set("fill_in_limit", (double)v); }
  float_t get_fill_in_limit() const { return (float_t)get_real("fill_in_limit"); }
  bool get_verbose() const { return get("verbose") != 0; }
  void set_verbose(const bool v) { set("verbose", v ? 1 : 0); }
  bool get_async_update() const { return get("async_update") != 0; }
  void set_async_update(const bool v) { set("async_update", v ? 1 : 0); }
  int get_num_iters() const { return (int)get("num_iters"); }
  nnz_scalar_t get_end_rel_res() const { return (nnz_scalar_t)get_real("end_rel_res"); }
  // the library's knobs and counters (kkamd_par_ilut_set / _get / _get_real)
  void set(const char* key, double value) { KokkosSparse::Impl::kkamd_check(kkamd_par_ilut_set(h_, key, value)); }
  int64_t get(const char* key) const { int64_t v = 0; KokkosSparse::Impl::kkamd_check(kkamd_par_ilut_get(h_, key, &v)); return v; }
  double get_real(const char* key) const { double v = 0; KokkosSparse::Impl::kkamd_check(kkamd_par_ilut_get_real(h_, key, &v)); return v; }

 private:
  bool reset_ = false;
  int team_size = -1, vector_size = -1;
  kkamd_par_ilut_handle_t* h_ = nullptr;
};

}}  // namespace KokkosSparse::Experimental
