// dune-hdd_amd/csrc/host/hdd_internal.hh -- error plumbing shared by the host and device halves of the ABI.
// The reference reports failures with DUNE_THROW (swipdg.hh:173-176, base.hh:285-289); across the C ABI
// they become status codes plus a per-thread message (hdd_last_error).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "hdd.h"

namespace hdd {
std::string& last_error_slot();
// name of the assembly kernel the last hdd_swipdg_assemble call on this thread launched (hdd_last_tile_kernel; every
// launch path sets it, element-list side passes keep the tile launch's): static strings only
const char*& last_tile_kernel_slot();
int set_error(int code, const std::string& msg);
int ctx_device(const hdd_ctx* ctx);   // HIP device ordinal a context is bound to
int local_elem_type(const hdd_local* l);   // HDD_SIMPLEX | HDD_CUBE | HDD_HEX of the grid behind a local view

// Host tables of the ESV2007 estimator (hdd_estimator_create; estimator_tables.cpp), from the host view alone: the
// vertex -> DoF CSR (DoF 3 e + i of every element e with local vertex i at the vertex, ascending) and the flags of the
// vertices on a boundary face, in the vertex numbering of hdd_local_vertices.  Rejects what the estimator does not
// cover (HDD_ERR_UNSUPPORTED: no 2d simplex grid, a view with ghosts, a Neumann face, 3 n_local >= 2^31).
struct EstimatorTables {
  int64_t n_local = 0, n_vertices = 0;
  std::vector<int64_t> patch_ptr;
  std::vector<int32_t> patch_dof;
  std::vector<uint8_t> vertex_bnd;
  std::vector<int32_t> elem_vertices;   // [3][n_local]: kept for the segment diameters (hdd_estimator_set_segments)
  std::vector<double> vertex_coords;    // [n_vertices][2]
};
int estimator_tables(const hdd_local* l, EstimatorTables* out);

// Per-segment tables of the OS2014 block estimator (hdd_estimator_set_segments), from host element bounds
// [n_segments + 1] (strictly ascending, bounds[0] == 0, bounds[S] == n_local; HDD_ERR_INVALID otherwise): the bounds,
// the number of 256-element chunks before each segment, and diam_s, the largest distance between two vertices of the
// segment's elements -- the pairwise maximum over the convex hull of the segment's distinct vertices (monotone
// chain), O(V log V) where the reference's loop (block-swipdg.hh:293-303) is O(V^2).
struct SegmentTables {
  std::vector<int64_t> bounds, chunk_prefix;
  std::vector<double> diam;
};
// every component > 0 (false for a NaN: this lives in host code built without -ffinite-math-only)
bool theta_positive(int32_t n_comp, const double* theta);
int estimator_segment_tables(int64_t n_local, int64_t n_vertices, const int32_t* elem_vertices, const double* vertex_coords,
                             int64_t n_segments, const int64_t* bounds, SegmentTables* out);
}  // namespace hdd

// Sharded-step fixup off the assembly stream (abi_assemble.hip, used by shard_step.hip): the element-list pass into side
// buffers of hdd_fix_rb(elem_type) doubles per listed element (n + 1 slots per component), and the copy of those
// row blocks into the value arrays.
int hdd_fix_rb(int32_t elem_type);
int hdd_assemble_elements_buf(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                              const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                              double* const* d_bufs, const int32_t* d_elems, int64_t n_elems, void* stream);
int hdd_scatter_fix(hdd_ctx* ctx, const hdd_csr* pattern, int32_t rb, double* const* d_bufs, int32_t n_comp,
                    const int32_t* d_elems, int64_t n_elems, double* const* d_vals, void* stream);
// Q1 side buffers in value-major (SoA) order: value k (canonical: row i, block b, column c, k = 20 i + 4 b + c) of
// listed element j at d_bufs[c][k ld + j] (coalesced element-pass stores), put into place by a wave per element;
// and a full-range launch that leaves reserve_wg workgroup slots to that element pass
int hdd_assemble_elements_soa(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                              const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                              double* const* d_bufs, int64_t ld, const int32_t* d_elems, int64_t n_elems, void* stream);
int hdd_scatter_fix_q1_soa(hdd_ctx* ctx, const hdd_mesh* m, const hdd_csr* pattern, double* const* d_bufs, int64_t ld,
                           int32_t n_comp, const int32_t* d_elems, int64_t n_elems, double* const* d_vals, void* stream);
int hdd_assemble_reserve(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                         const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                         double* const* d_vals, void* stream, int32_t reserve_wg);
// the same pass in place (no side buffer), beside a full-range assembly that skips those elements' row blocks
int hdd_assemble_elements_inplace(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                                  const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                                  double* const* d_vals, const int32_t* d_elems, int64_t n_elems, void* stream);
// reserve_wg: workgroups of the concurrent element pass (in-place fixup) -- the persistent launch leaves that many
// slots free when its own tiles would fill the CUs (launch_persistent)
int hdd_assemble_skip_ghost(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                            const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                            double* const* d_vals, void* stream, int32_t reserve_wg = 0);
