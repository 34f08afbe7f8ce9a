// KokkosKernels::Experimental::KokkosKernelsHandle -- the slice the SpGEMM, SPTRSV, SPILUK, Gauss-Seidel, GMRES and PAR_ILUT paths use
// (reference: sparse/src/KokkosKernels_Handle.hpp:37-66,281-343,380-482, sptrsv :765-783,848-862, spiluk :853-870, gauss-seidel :538-544,581-628,
// 715-720): create / get / destroy of the SpGEMM, SPTRSV, SPILUK and Gauss-Seidel sub-handles plus the tuning setters.  set_verbose acts (the library prints the chosen algorithm, row bins and compression
// decision, like KOKKOSKERNELS_VERBOSE).  The team / vector / shared-memory / scheduling setters are HINTS in the reference
// too -- its rocSPARSE and cuSPARSE paths take and ignore them, and its driver and unit tests set them before every spgemm
// (perf_test/sparse/KokkosSparse_spgemm.cpp:311-317, sparse/unit_test/Test_Sparse_spgemm.hpp:91-92) -- so they are accepted,
// remembered (the get_set_* getters of the reference return them), forwarded to the library as recorded hints (reported
// under verbose) and have no effect: launch shapes and LDS tables follow the row bins.
#pragma once
#include "KokkosSparse_spgemm_handle.hpp"
#include "KokkosSparse_sptrsv_handle.hpp"
#include "KokkosSparse_spiluk_handle.hpp"
#include "KokkosSparse_gauss_seidel_handle.hpp"
#include "KokkosSparse_gmres_handle.hpp"
#include "KokkosSparse_par_ilut_handle.hpp"

namespace KokkosKernels { namespace Experimental {

template <class size_type_, class lno_t_, class scalar_t_, class ExecutionSpace, class TemporaryMemorySpace,
          class PersistentMemorySpace>
class KokkosKernelsHandle {
 public:
  using size_type        = std::remove_const_t<size_type_>;
  using nnz_lno_t        = std::remove_const_t<lno_t_>;
  using nnz_scalar_t     = std::remove_const_t<scalar_t_>;
  using const_size_type  = const size_type;
  using const_nnz_lno_t  = const nnz_lno_t;
  using const_nnz_scalar_t = const nnz_scalar_t;
  using HandleExecSpace  = ExecutionSpace;
  using HandleTempMemorySpace       = TemporaryMemorySpace;
  using HandlePersistentMemorySpace = PersistentMemorySpace;
  using SPGEMMHandleType = KokkosSparse::SPGEMMHandle<size_type, nnz_lno_t, nnz_scalar_t, ExecutionSpace,
                                                     TemporaryMemorySpace, PersistentMemorySpace>;
  using SPTRSVHandleType = KokkosSparse::Experimental::SPTRSVHandle<size_type, nnz_lno_t, nnz_scalar_t, ExecutionSpace,
                                                                   TemporaryMemorySpace, PersistentMemorySpace>;
  using SPILUKHandleType = KokkosSparse::Experimental::SPILUKHandle<size_type, nnz_lno_t, nnz_scalar_t, ExecutionSpace,
                                                                   TemporaryMemorySpace, PersistentMemorySpace>;
  using GaussSeidelHandleType = KokkosSparse::GaussSeidelHandle<size_type, nnz_lno_t, nnz_scalar_t, ExecutionSpace, TemporaryMemorySpace,
                                                               PersistentMemorySpace>;
  using PointGaussSeidelHandleType = KokkosSparse::PointGaussSeidelHandle<size_type, nnz_lno_t, nnz_scalar_t, ExecutionSpace, TemporaryMemorySpace,
                                                                         PersistentMemorySpace>;
  using GMRESHandleType = KokkosSparse::Experimental::GMRESHandle<size_type, nnz_lno_t, nnz_scalar_t, ExecutionSpace, TemporaryMemorySpace,
                                                                 PersistentMemorySpace>;
  using PAR_ILUTHandleType = KokkosSparse::Experimental::PAR_ILUTHandle<size_type, nnz_lno_t, nnz_scalar_t, ExecutionSpace, TemporaryMemorySpace,
                                                                       PersistentMemorySpace>;
  KokkosKernelsHandle() = default;
  ~KokkosKernelsHandle() { destroy_spgemm_handle(); destroy_sptrsv_handle(); destroy_spiluk_handle(); destroy_gs_handle(); destroy_gmres_handle(); destroy_par_ilut_handle(); }
  KokkosKernelsHandle(const KokkosKernelsHandle&)            = delete;
  KokkosKernelsHandle& operator=(const KokkosKernelsHandle&) = delete;

  void create_spgemm_handle(KokkosSparse::SPGEMMAlgorithm algo = KokkosSparse::SPGEMM_DEFAULT) {
    destroy_spgemm_handle();
    spgemm_ = new SPGEMMHandleType(algo);
    if (verbose_) spgemm_->set_verbose(true);
    // hints given before the sub-handle existed (the reference's order: setters first, then create_spgemm_handle)
    if (team_work_size != -1) spgemm_->set("team_work_size", team_work_size);
    if (shared_memory_size != 16128) spgemm_->set("shmem_size", (double)shared_memory_size);
    if (suggested_team_size != -1) spgemm_->set("suggested_team_size", suggested_team_size);
    if (vector_size != -1) spgemm_->set("suggested_vector_size", vector_size);
    if (!use_dynamic_scheduling) spgemm_->set("dynamic_scheduling", 0);
  }
  SPGEMMHandleType* get_spgemm_handle() { return spgemm_; }
  void destroy_spgemm_handle() { delete spgemm_; spgemm_ = nullptr; }

  // SPTRSV sub-handle (:765-783,848-862); the hints given to this handle go to it as in the reference (:773-774)
  SPTRSVHandleType* get_sptrsv_handle() { return sptrsv_; }
  void create_sptrsv_handle(KokkosSparse::Experimental::SPTRSVAlgorithm algm, size_type nrows, bool lower_tri, size_type block_size = 0) {
    destroy_sptrsv_handle();
    sptrsv_ = new SPTRSVHandleType(algm, nrows, lower_tri, block_size);
    sptrsv_->set_team_size(team_work_size);
    sptrsv_->set_vector_size(vector_size);
  }
  void destroy_sptrsv_handle() { delete sptrsv_; sptrsv_ = nullptr; }
  bool is_sptrsv_lower_tri() { return sptrsv_->is_lower_tri(); }

  // SPILUK sub-handle (:853-870); nnzL and nnzU are the caller's estimates until the symbolic phase sets the true counts
  SPILUKHandleType* get_spiluk_handle() { return spiluk_; }
  void create_spiluk_handle(KokkosSparse::Experimental::SPILUKAlgorithm algm, size_type nrows, size_type nnzL, size_type nnzU,
                            size_type block_size = 0) {
    destroy_spiluk_handle();
    spiluk_ = new SPILUKHandleType(algm, nrows, nnzL, nnzU, block_size);
    spiluk_->set_team_size(team_work_size);
    spiluk_->set_vector_size(vector_size);
  }
  void destroy_spiluk_handle() { delete spiluk_; spiluk_ = nullptr; }

  // Gauss-Seidel sub-handle (:538-544,581-628,715-720).  The reference's second argument, the colouring algorithm, does not exist here:
  // the library colours with its own deterministic Jones-Plassmann (include/kkamd.h).  GS_CLUSTER / GS_TWOSTAGE throw std::runtime_error.
  GaussSeidelHandleType* get_gs_handle() { return gs_; }
  PointGaussSeidelHandleType* get_point_gs_handle() { return gs_; }
  void create_gs_handle(KokkosSparse::GSAlgorithm gs_algorithm = KokkosSparse::GS_DEFAULT) {
    destroy_gs_handle();
    gs_ = new PointGaussSeidelHandleType(gs_algorithm);
  }
  void destroy_gs_handle() { delete gs_; gs_ = nullptr; }

  // GMRES sub-handle (reference: sparse/src/KokkosKernels_Handle.hpp, create_gmres_handle(m, tol, max_restart) / get / destroy)
  GMRESHandleType* get_gmres_handle() { return gmres_; }
  void create_gmres_handle(const size_type m = 50, const typename GMRESHandleType::float_t tol = 1e-8, const size_type max_restart = 50) {
    destroy_gmres_handle();
    gmres_ = new GMRESHandleType(m, tol, max_restart);
  }
  void destroy_gmres_handle() { delete gmres_; gmres_ = nullptr; }

  // PAR_ILUT sub-handle (:871-881, the reference's defaults); the hints given to this handle go to it as in the reference
  PAR_ILUTHandleType* get_par_ilut_handle() { return par_ilut_; }
  void create_par_ilut_handle(const size_type max_iter = 20, const typename PAR_ILUTHandleType::float_t residual_norm_delta_stop = 1e-2,
                              const typename PAR_ILUTHandleType::float_t fill_in_limit = 0.75, const bool async_update = false,
                              const bool verbose = false) {
    destroy_par_ilut_handle();
    par_ilut_ = new PAR_ILUTHandleType(max_iter, residual_norm_delta_stop, fill_in_limit, async_update, verbose);
    par_ilut_->set_team_size(team_work_size);
    par_ilut_->set_vector_size(vector_size);
  }
  void destroy_par_ilut_handle() { delete par_ilut_; par_ilut_ = nullptr; }

  // hints of the reference (:380-465; defaults :203-215): remembered, forwarded, without effect on gfx950
  void set_team_work_size(const int v) { team_work_size = v; hint("team_work_size", v); }
  int get_set_team_work_size() { return team_work_size; }
  int get_team_work_size(const int team_size, const int /*concurrency*/, const nnz_lno_t /*overall_work_size*/) {
    return team_work_size != -1 ? team_work_size : team_size;                      // the reference's answer for Exec_HIP (:393-404)
  }
  void set_shmem_size(const size_t v) { shared_memory_size = v; hint("shmem_size", (double)v); }
  size_t get_shmem_size() { return shared_memory_size; }
  void set_suggested_team_size(const int v) { suggested_team_size = v; hint("suggested_team_size", v); }
  int get_set_suggested_team_size() { return suggested_team_size; }
  void set_suggested_vector_size(int v) { vector_size = v; hint("suggested_vector_size", v); }
  int get_set_suggested_vector_size() { return vector_size; }
  void set_dynamic_scheduling(const bool v) { use_dynamic_scheduling = v; hint("dynamic_scheduling", v ? 1 : 0); }
  bool is_dynamic_scheduling() { return use_dynamic_scheduling; }
  void set_verbose(bool v) { verbose_ = v; if (spgemm_) spgemm_->set_verbose(v); }
  bool get_verbose() const { return verbose_; }
 private:
  void hint(const char* key, double v) { if (spgemm_) spgemm_->set(key, v); }
  int team_work_size        = -1;        // the reference's defaults (:203-215)
  size_t shared_memory_size = 16128;
  int suggested_team_size   = -1;
  int vector_size           = -1;
  bool use_dynamic_scheduling = true;
  SPGEMMHandleType* spgemm_ = nullptr;
  SPTRSVHandleType* sptrsv_ = nullptr;
  SPILUKHandleType* spiluk_ = nullptr;
  PointGaussSeidelHandleType* gs_ = nullptr;
  GMRESHandleType* gmres_   = nullptr;
  PAR_ILUTHandleType* par_ilut_ = nullptr;
  bool verbose_             = false;
};

}}  // namespace KokkosKernels::Experimental
