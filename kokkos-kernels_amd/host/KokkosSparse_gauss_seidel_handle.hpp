// GSAlgorithm / GSDirection / GaussSeidelHandle / PointGaussSeidelHandle -- reference: sparse/src/KokkosSparse_gauss_seidel_handle.hpp:30-31
// (the enums), :34-260 (GaussSeidelHandle), :262-450 (PointGaussSeidelHandle, set_long_row_threshold :346).  The colours, the
// permutation, the permuted matrix, the inverse diagonal and the permuted work vectors live in the library's kkamd_gs_handle; this
// class forwards to it.  GS_DEFAULT, GS_PERMUTED and GS_TEAM run the library's multicolor sweep (GS_PERMUTED with one lane per row);
// GS_CLUSTER and GS_TWOSTAGE throw at construction.  There is one handle class: point Gauss-Seidel is all there is, so
// GaussSeidelHandle is an alias of PointGaussSeidelHandle.
#pragma once
#include <string>
#include <vector>
#include "Kokkos_Shim.hpp"
#include "kkamd_status.hpp"

namespace KokkosSparse {

enum GSAlgorithm { GS_DEFAULT, GS_PERMUTED, GS_TEAM, GS_CLUSTER, GS_TWOSTAGE };
enum GSDirection { GS_FORWARD, GS_BACKWARD, GS_SYMMETRIC };
// sparse/src/KokkosSparse_Utils.hpp:37-40: the format parameter of the Gauss-Seidel entry points; CRS is what is implemented
enum class SparseMatrixFormat { BSR, CRS };

template <class size_type_, class lno_t_, class scalar_t_, class ExecutionSpace, class TemporaryMemorySpace,
          class PersistentMemorySpace>
class PointGaussSeidelHandle {
 public:
  using HandleExecSpace             = ExecutionSpace;
  using HandleTempMemorySpace       = TemporaryMemorySpace;
  using HandlePersistentMemorySpace = PersistentMemorySpace;
  using size_type                   = std::remove_const_t<size_type_>;
  using nnz_lno_t                   = std::remove_const_t<lno_t_>;
  using nnz_scalar_t                = std::remove_const_t<scalar_t_>;

  explicit PointGaussSeidelHandle(GSAlgorithm gs = GS_DEFAULT) : algorithm_type(gs) { Impl::kkamd_check(kkamd_gs_create(&h_, (int)gs)); }
  virtual ~PointGaussSeidelHandle() { if (h_) kkamd_gs_destroy(h_); }
  PointGaussSeidelHandle(const PointGaussSeidelHandle&)            = delete;
  PointGaussSeidelHandle& operator=(const PointGaussSeidelHandle&) = delete;

  kkamd_gs_handle_t* native() const { return h_; }
  GSAlgorithm get_algorithm_type() const { return algorithm_type; }
  bool is_symbolic_called() const { return get("symbolic_complete") != 0; }
  bool is_numeric_called() const { return get("numeric_complete") != 0; }
  nnz_lno_t get_num_colors() const { return (nnz_lno_t)get("num_colors"); }
  void set_long_row_threshold(nnz_lno_t lrt) { set("long_row_threshold", (int)lrt); }
  nnz_lno_t get_long_row_threshold() const { return (nnz_lno_t)get("long_row_threshold"); }
  nnz_lno_t get_num_long_rows() const { return (nnz_lno_t)get("long_rows"); }
  // the library's knobs and counters (kkamd_gs_set / _get) and the colouring as host arrays (kkamd_gs_export)
  void set(const char* key, int value) { Impl::kkamd_check(kkamd_gs_set(h_, key, value)); }
  int64_t get(const char* key) const { int64_t v = 0; Impl::kkamd_check(kkamd_gs_get(h_, key, &v)); return v; }
  std::vector<int> export_host(const char* what) const {
    std::vector<int> out((size_t)(std::string(what) == "color_xadj" ? get("num_colors") + 1 : get("num_rows")));
    Impl::kkamd_check(kkamd_gs_export(h_, what, out.data(), (int64_t)out.size()));
    return out;
  }
 private:
  GSAlgorithm algorithm_type;
  kkamd_gs_handle_t* h_ = nullptr;
};

template <class size_type_, class lno_t_, class scalar_t_, class ExecutionSpace, class TemporaryMemorySpace,
          class PersistentMemorySpace>
using GaussSeidelHandle = PointGaussSeidelHandle<size_type_, lno_t_, scalar_t_, ExecutionSpace, TemporaryMemorySpace, PersistentMemorySpace>;

}  // namespace KokkosSparse
