// SPTRSVAlgorithm / SPTRSVHandle -- reference: sparse/src/KokkosSparse_sptrsv_handle.hpp:42-52,54-63,407-,859-960.
// The level sets (level_list, nodes_per_level, nodes_grouped_by_level), the diagonal positions and the launch plan live in the
// library's kkamd_sptrsv_handle; this class forwards to it.  The three level-scheduled algorithm values run the library's kernels
// (RP one lane per row, TP1 lanes chosen per level, TP1CHAIN the same with narrow levels chained); SPTRSV_CUSPARSE throws at
// construction, the supernodal values do not exist here.  set_team_size / set_vector_size are hints in the reference's own TPL path
// and are remembered without effect; set_vector_size with a power of two up to 64 pins the lanes per row.
#pragma once
#include <string>
#include <vector>
#include "Kokkos_Shim.hpp"
#include "kkamd_status.hpp"

namespace KokkosSparse { namespace Experimental {

enum class SPTRSVAlgorithm { SEQLVLSCHD_RP, SEQLVLSCHD_TP1, SEQLVLSCHD_TP1CHAIN, SPTRSV_CUSPARSE };

inline SPTRSVAlgorithm StringToSPTRSVAlgorithm(const std::string& name) {
  if (name == "SPTRSV_DEFAULT" || name == "SPTRSV_SEQLVLSCHD_RP" || name == "SEQLVLSCHD_RP") return SPTRSVAlgorithm::SEQLVLSCHD_RP;
  if (name == "SPTRSV_SEQLVLSCHD_TP1" || name == "SEQLVLSCHD_TP1") return SPTRSVAlgorithm::SEQLVLSCHD_TP1;
  if (name == "SPTRSV_SEQLVLSCHD_TP1CHAIN" || name == "SEQLVLSCHD_TP1CHAIN") return SPTRSVAlgorithm::SEQLVLSCHD_TP1CHAIN;
  if (name == "SPTRSV_CUSPARSE") return SPTRSVAlgorithm::SPTRSV_CUSPARSE;
  throw std::runtime_error("Invalid SPTRSVAlgorithm name");
}

template <class size_type_, class lno_t_, class scalar_t_, class ExecutionSpace, class TemporaryMemorySpace,
          class PersistentMemorySpace>
class SPTRSVHandle {
 public:
  using HandleExecSpace             = ExecutionSpace;
  using HandleTempMemorySpace       = TemporaryMemorySpace;
  using HandlePersistentMemorySpace = PersistentMemorySpace;
  using execution_space             = ExecutionSpace;
  using memory_space                = HandlePersistentMemorySpace;
  using size_type                   = std::remove_const_t<size_type_>;
  using nnz_lno_t                   = std::remove_const_t<lno_t_>;
  using scalar_t                    = std::remove_const_t<scalar_t_>;
  using signed_integral_t           = std::make_signed_t<size_type>;

  SPTRSVHandle(SPTRSVAlgorithm choice, const size_type nrows_, bool lower_tri_, const size_type block_size_ = 0) : algm(choice) {
    if (block_size_ != 0) throw std::runtime_error("KokkosSparse::SPTRSVHandle: block (BSR) sptrsv is not supported");
    Impl::kkamd_check(kkamd_sptrsv_create(&h_, (int)choice, (int64_t)nrows_, lower_tri_ ? 1 : 0));
  }
  virtual ~SPTRSVHandle() { if (h_) kkamd_sptrsv_destroy(h_); }
  SPTRSVHandle(const SPTRSVHandle&)            = delete;
  SPTRSVHandle& operator=(const SPTRSVHandle&) = delete;

  kkamd_sptrsv_handle_t* native() const { return h_; }
  SPTRSVAlgorithm get_algorithm() { return algm; }
  size_type get_nrows() const { return (size_type)get("num_rows"); }
  bool is_lower_tri() const { return get("lower_tri") != 0; }
  bool is_upper_tri() const { return !is_lower_tri(); }
  bool is_symbolic_complete() const { return get("symbolic_complete") != 0; }
  size_type get_num_levels() const { return (size_type)get("num_levels"); }
  // a level with at most this many rows may join a chain (SEQLVLSCHD_TP1CHAIN); the reference's chain threshold (:900-924)
  void reset_chain_threshold(const signed_integral_t threshold) { set("chain_rows", (int)threshold); }
  signed_integral_t get_chain_threshold() const { return (signed_integral_t)get("chain_rows"); }
  void set_team_size(const int ts) { team_size = ts; }
  int get_team_size() const { return team_size; }
  void set_vector_size(const int vs) {
    vector_size = vs;
    if (vs >= 1 && vs <= 64 && (vs & (vs - 1)) == 0) set("lanes_per_row", vs);
  }
  int get_vector_size() const { return vector_size; }
  // the library's knobs and counters (kkamd_sptrsv_set / _get) and the level sets as host arrays (kkamd_sptrsv_export)
  void set(const char* key, int value) { Impl::kkamd_check(kkamd_sptrsv_set(h_, key, value)); }
  int64_t get(const char* key) const { int64_t v = 0; Impl::kkamd_check(kkamd_sptrsv_get(h_, key, &v)); return v; }
  std::vector<int> export_host(const char* what) const {
    std::vector<int> out((size_t)(std::string(what) == "nodes_per_level" ? get("num_levels") : get("num_rows")));
    Impl::kkamd_check(kkamd_sptrsv_export(h_, what, out.data(), (int64_t)out.size()));
    return out;
  }
 private:
  SPTRSVAlgorithm algm;
  int team_size = -1, vector_size = -1;
  kkamd_sptrsv_handle_t* h_ = nullptr;
};

}}  // namespace KokkosSparse::Experimental
