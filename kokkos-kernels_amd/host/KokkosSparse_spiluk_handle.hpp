// SPILUKAlgorithm / SPILUKHandle -- reference: sparse/src/KokkosSparse_spiluk_handle.hpp:31-33,35-247.
// The level sets of L (level_list, level_ptr, level_idx) and the launch plan live in the library's kkamd_spiluk_handle; this class
// forwards to it.  Kept from the reference, as far as it means something here: get_ / set_nnzL and nnzU (callers size and resize
// their views by them; the symbolic phase sets the true counts), get_nrows, get_num_levels, get_level_maxrows,
// is_symbolic_complete / reset_symbolic_complete, reset_handle, get_ / set_algorithm, print_algorithm, and set_team_size /
// set_vector_size (hints; set_vector_size with a power of two up to 64 pins the lanes per row).  Not here: the block (BSR) variant
// (block_size > 0 throws), the chunking of levels and the dense iw work array (alloc_iw, level_nchunks, level_nrowsperchunk), which
// the library's kernels do not need.
#pragma once
#include <iostream>
#include <limits>
#include <string>
#include <vector>
#include "Kokkos_Shim.hpp"
#include "kkamd_status.hpp"

namespace KokkosSparse { namespace Experimental {

enum class SPILUKAlgorithm { SEQLVLSCHD_TP1 };

template <class size_type_, class lno_t_, class scalar_t_, class ExecutionSpace, class TemporaryMemorySpace,
          class PersistentMemorySpace>
class SPILUKHandle {
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

  SPILUKHandle(SPILUKAlgorithm choice, const size_type nrows_, const size_type nnzL_, const size_type nnzU_, const size_type block_size_ = 0)
      : algm(choice) {
    create(nrows_, nnzL_, nnzU_, block_size_);
  }
  virtual ~SPILUKHandle() { if (h_) kkamd_spiluk_destroy(h_); }
  SPILUKHandle(const SPILUKHandle&)            = delete;
  SPILUKHandle& operator=(const SPILUKHandle&) = delete;

  // a new analysis state for a matrix of another size (:123-144); the knobs go back to their defaults
  void reset_handle(const size_type nrows_, const size_type nnzL_, const size_type nnzU_,
                    const size_type block_size_ = std::numeric_limits<size_type>::max()) {
    kkamd_spiluk_handle_t* old = h_;
    h_ = nullptr;
    try { create(nrows_, nnzL_, nnzU_, block_size_ == std::numeric_limits<size_type>::max() ? 0 : block_size_); }
    catch (...) { h_ = old; throw; }
    if (old) kkamd_spiluk_destroy(old);
    if (vector_size >= 1) set_vector_size(vector_size);
  }

  kkamd_spiluk_handle_t* native() const { return h_; }
  void set_algorithm(SPILUKAlgorithm choice) { algm = choice; }
  SPILUKAlgorithm get_algorithm() { return algm; }
  size_type get_nrows() const { return (size_type)get("num_rows"); }
  size_type get_nnzL() const { return nnzL; }
  void set_nnzL(const size_type nnzL_) { nnzL = nnzL_; }
  size_type get_nnzU() const { return nnzU; }
  void set_nnzU(const size_type nnzU_) { nnzU = nnzU_; }
  size_type get_block_size() const { return 0; }
  bool is_block_enabled() const { return false; }
  size_type get_level_maxrows() const { return (size_type)get("max_level_rows"); }
  size_type get_num_levels() const { return (size_type)get("num_levels"); }
  bool is_symbolic_complete() const { return !reset_ && get("symbolic_complete") != 0; }
  void reset_symbolic_complete() { reset_ = true; }
  void set_team_size(const int ts) { team_size = ts; }
  int get_team_size() const { return team_size; }
  void set_vector_size(const int vs) {
    vector_size = vs;
    if (vs >= 1 && vs <= 64 && (vs & (vs - 1)) == 0) set("lanes_per_row", vs);
  }
  int get_vector_size() const { return vector_size; }
  void print_algorithm() { std::cout << "SEQLVLSCHD_TP1" << std::endl; }
  // the library's knobs and counters (kkamd_spiluk_set / _get) and the level sets as host arrays (kkamd_spiluk_export)
  void set(const char* key, int value) { Impl::kkamd_check(kkamd_spiluk_set(h_, key, value)); }
  int64_t get(const char* key) const { int64_t v = 0; Impl::kkamd_check(kkamd_spiluk_get(h_, key, &v)); return v; }
  std::vector<int> export_host(const char* what) const {
    std::vector<int> out((size_t)(std::string(what) == "level_ptr" ? get("num_levels") + 1 : get("num_rows")));
    Impl::kkamd_check(kkamd_spiluk_export(h_, what, out.data(), (int64_t)out.size()));
    return out;
  }
  // called by spiluk_symbolic: the true counts replace the caller's estimates (symbolic_impl.hpp:391-392)
  void symbolic_done() { nnzL = (size_type)get("nnzL"); nnzU = (size_type)get("nnzU"); reset_ = false; }

 private:
  void create(size_type nrows_, size_type nnzL_, size_type nnzU_, size_type block_size_) {
    if (block_size_ != 0) throw std::runtime_error("KokkosSparse::SPILUKHandle: block (BSR) spiluk is not supported");
    Impl::kkamd_check(kkamd_spiluk_create(&h_, KKAMD_SPILUK_SEQLVLSCHD_TP1, (int64_t)nrows_, (int64_t)nnzL_, (int64_t)nnzU_));
    nnzL = nnzL_; nnzU = nnzU_; reset_ = false;
  }
  SPILUKAlgorithm algm;
  size_type nnzL = 0, nnzU = 0;
  bool reset_ = false;
  int team_size = -1, vector_size = -1;
  kkamd_spiluk_handle_t* h_ = nullptr;
};

}}  // namespace KokkosSparse::Experimental
