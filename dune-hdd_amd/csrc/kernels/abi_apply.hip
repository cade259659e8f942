// dune-hdd_amd/csrc/kernels/abi_apply.hip -- C ABI: operator application on the assembled value arrays
// (hdd_operator_apply, hdd_operator_apply_multi, hdd_operator_apply2; kernels in apply_kernels.hh): what pyMOR's apply / apply2 and LRBMS's
// local / coupling operators need from the containers SWIPDG::init() fills (base.hh:45, 260-264, 327-367;
// block-swipdg.hh:625-676), on the device, with the theta-lincomb fused and block ranges applied in place.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "apply_plan.hh"

using hdd::set_error;
using hdd::abi::ApplyPlan;
using hdd::abi::fail;
using hdd::abi::plan_apply;
using hdd::abi::run_apply;
using hdd::abi::ApplyThetas;
namespace dev = hdd::dev;

namespace {
std::string& last_apply_kernel_slot()
{
  thread_local std::string name;
  return name;
}
}  // namespace

int hdd::abi::plan_apply(const char* who, hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
               int32_t n_comp, const double* theta, const hdd_block_range* range, ApplyPlan& P, bool per_vector)
{
  if (!ctx || !pattern || !d_vals) return fail(HDD_ERR_INVALID, who, "null argument");
  if (n_comp < 1 || n_comp > HDD_MAX_COMP) return fail(HDD_ERR_INVALID, who, "n_comp outside 1..HDD_MAX_COMP");
  for (int q = 0; q < n_comp; ++q)
    if (!d_vals[q]) return fail(HDD_ERR_INVALID, who, "null value array");
  if (pattern->n_rows < 0 || pattern->n_cols < 0 || pattern->nnz < 0) return fail(HDD_ERR_INVALID, who, "negative pattern sizes");
  hdd_block_range rg{0, pattern->n_rows, 0, pattern->n_cols};
  if (range) rg = *range;
  if (rg.row_begin < 0 || rg.row_begin > rg.row_end || rg.row_end > pattern->n_rows || rg.col_begin < 0 ||
      rg.col_begin > rg.col_end || rg.col_end > pattern->n_cols)
    return fail(HDD_ERR_INVALID, who, "range outside the matrix");
  dev::ApplyArgs& a = P.a;
  a = dev::ApplyArgs{};
  a.n_comp = n_comp;
  bool aligned16 = true;
  for (int q = 0; q < n_comp; ++q) {
    a.vals[q] = d_vals[q];
    a.theta[q] = theta ? theta[q] : 1.0;
    aligned16 &= reinterpret_cast<uintptr_t>(d_vals[q]) % 16 == 0;
  }
  a.nnz = pattern->nnz;
  a.row_ptr = pattern->row_ptr;
  a.col = pattern->col;
  a.row_begin = rg.row_begin;
  a.row_end = rg.row_end;
  a.col_begin = rg.col_begin;
  a.col_end = rg.col_end;
  P.tile = false;
  if (mesh) {
    if (!hdd::abi::mesh_faces(mesh->elem_type)) return fail(HDD_ERR_INVALID, who, "unknown element type");
    if (mesh->own_begin < 0 || mesh->own_end > mesh->n_local || mesh->own_begin > mesh->own_end)
      return fail(HDD_ERR_INVALID, who, "0 <= own_begin <= own_end <= n_local violated");
    if (!mesh->neighbors) return fail(HDD_ERR_INVALID, who, "mesh without neighbors");
    const bool two_d = (mesh->elem_type == HDD_SIMPLEX || mesh->elem_type == HDD_CUBE) && mesh->degree <= 1;
    const int nb = two_d ? hdd::abi::mesh_nb(mesh->elem_type, 1) : 0;
    if (two_d && pattern->n_rows != int64_t(nb) * (mesh->own_end - mesh->own_begin))
      return fail(HDD_ERR_INVALID, who, "pattern rows != nb * owned elements of the mesh");
    // the tile kernel: local == global numbering, nb-aligned range, aligned value stream, 32-bit byte offsets into x
    if (two_d && pattern->elem_ptr && pattern->n_cols == int64_t(nb) * mesh->n_local && aligned16 &&
        rg.row_begin % nb == 0 && rg.row_end % nb == 0 && rg.col_begin % nb == 0 && rg.col_end % nb == 0 &&
        rg.col_end - rg.col_begin < (int64_t(1) << 29) && mesh->n_local < (int64_t(1) << 31)) {
      P.tile = true;
      P.nb = nb;
      P.nf = hdd::abi::mesh_faces(mesh->elem_type);
      a.elem_ptr = pattern->elem_ptr;
      a.nbrs = mesh->neighbors;
      a.n_local = mesh->n_local;
      a.own_begin = mesh->own_begin;
      a.e_begin = mesh->own_begin + rg.row_begin / nb;
      a.e_end = mesh->own_begin + rg.row_end / nb;
      a.ce_begin = rg.col_begin / nb;
      a.ce_end = rg.col_end / nb;
    }
  }
  // the generic path -- also with a theta per vector where the component images do not fit the LDS
  const bool no_images = per_vector && P.tile && !(P.nb == 3 ? n_comp <= 3 : n_comp == 1);
  if (!P.tile || no_images) {
    if (!pattern->row_ptr || !pattern->col)
      return fail(HDD_ERR_INVALID, who, no_images ? "pattern without row_ptr / col (component images beyond the LDS)" : "pattern without row_ptr / col");
    P.tile = false;
    P.short_rows = pattern->n_rows == 0 || pattern->nnz / std::max<int64_t>(pattern->n_rows, 1) <= 32;
  }
  return HDD_OK;
}

void hdd::abi::apply_multi_thetas(dev::ApplyMultiArgs& ma, const ApplyThetas& T, int v0)
{
  for (int v = 0; v < dev::APPLY_NV; ++v) {
    const int64_t j = v0 + (v < ma.a.nv ? v : 0);
    for (int q = 0; q < HDD_MAX_COMP; ++q) ma.theta[v][q] = q < ma.a.n_comp ? (T.theta ? T.theta[j * T.ldt + q] : 1.0) : 0.0;
  }
}

void hdd::abi::apply_kernel_name(std::string& out, const ApplyPlan& P, bool per_vector, int nv, bool dot)
{
  out += P.tile ? "apply_tile_" : "apply_csr_";
  out += per_vector ? "multi_kernel<" : "kernel<";
  out += P.tile ? (P.nb == 3 ? "3, 3, " : "4, 4, ") : (P.short_rows ? "8, " : "64, ");
  out += char('0' + nv);
  out += dot ? ", dot>" : ">";
}

void hdd::abi::name_project_kernel(const ApplyPlan& P)
{
  std::string& out = last_apply_kernel_slot();
  out = P.tile ? "project_tile_kernel<" : "project_csr_kernel<";
  out += P.tile ? (P.nb == 3 ? "3, 3>" : "4, 4>") : (P.short_rows ? "8>" : "64>");
}

int hdd::abi::run_apply(const char* who, hdd_ctx* ctx, const ApplyPlan& P, const ApplyThetas* T, const double* d_x, int64_t ldx,
                        double* d_y, int64_t ldy, int32_t n_vec, void* stream)
{
  if (P.rows() == 0) return HDD_OK;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int64_t grid = apply_grid(ctx, P);
  for (int v0 = 0; v0 < n_vec; v0 += dev::APPLY_NV) {
    dev::ApplyMultiArgs ma;
    dev::ApplyArgs& a = ma.a;
    a = P.a;
    a.nv = std::min<int>(dev::APPLY_NV, n_vec - v0);
    a.x = d_x + int64_t(v0) * ldx;
    a.ldx = ldx;
    a.y = d_y + int64_t(v0) * ldy;
    a.ldy = ldy;
    const int nv = T || a.nv > 1 ? dev::APPLY_NV : 1;   // the instantiation's
    last_apply_kernel_slot().clear();
    apply_kernel_name(last_apply_kernel_slot(), P, T != nullptr, nv, false);
    if (T) {
      apply_multi_thetas(ma, *T, v0);
      e = launch_apply<dev::APPLY_NV, false>(P, ma, grid, s);
    } else {
      e = nv > 1 ? launch_apply<dev::APPLY_NV, false>(P, a, grid, s) : launch_apply<1, false>(P, a, grid, s);
    }
    if (e != hipSuccess) return hip_fail(e, who);
  }
  return HDD_OK;
}

int hdd::abi::plan_blocks(const char* who, hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                          int32_t n_comp, const double* theta, int32_t n_blocks, const int64_t* bounds, ApplyPlan& P)
{
  if (!ctx || !pattern || !d_vals) return fail(HDD_ERR_INVALID, who, "null argument");
  if (n_blocks < 1 || n_blocks > HDD_MAX_SOLVE_BLOCKS) return fail(HDD_ERR_INVALID, who, "n_blocks outside 1..HDD_MAX_SOLVE_BLOCKS");
  if (!bounds) return fail(HDD_ERR_INVALID, who, "null bounds");
  for (int s = 0; s < n_blocks; ++s)
    if (bounds[s] >= bounds[s + 1]) return fail(HDD_ERR_INVALID, who, "bounds not strictly ascending");
  if (bounds[0] < 0 || bounds[n_blocks] > std::min(pattern->n_rows, pattern->n_cols))
    return fail(HDD_ERR_INVALID, who, "bounds outside the square part of the matrix");
  const hdd_block_range rg{bounds[0], bounds[n_blocks], bounds[0], bounds[n_blocks]};
  if (int rc = plan_apply(who, ctx, mesh, pattern, d_vals, n_comp, theta, &rg, P)) return rc;
  bool aligned = true;
  for (int s = 1; P.tile && s < n_blocks; ++s) aligned = aligned && bounds[s] % P.nb == 0;
  // a segment that begins inside an element: what the single call on its range does
  return aligned ? HDD_OK : plan_apply(who, ctx, nullptr, pattern, d_vals, n_comp, theta, &rg, P);
}

void hdd::abi::blocks_table(const hdd_ctx* ctx, const ApplyPlan& P, int32_t n_blocks, const int64_t* bounds, int block_size,
                            int64_t max_parts, dev::BlockSegment* tab, int64_t (&total)[dev::BLOCKS_KINDS])
{
  for (int64_t& t : total) t = 0;
  for (int s = 0; s < n_blocks; ++s) {
    dev::BlockSegment& g = tab[s];
    ApplyPlan Q = P;   // the plan of a call on this segment's range
    dev::ApplyArgs& a = Q.a;
    a.row_begin = a.col_begin = bounds[s];
    a.row_end = a.col_end = bounds[s + 1];
    if (P.tile) {
      a.e_begin = a.own_begin + bounds[s] / P.nb;
      a.e_end = a.own_begin + bounds[s + 1] / P.nb;
      a.ce_begin = bounds[s] / P.nb;
      a.ce_end = bounds[s + 1] / P.nb;
    }
    const int64_t rows = Q.rows();
    g.row_begin = a.row_begin;
    g.rows = rows;
    g.e_begin = a.e_begin;
    g.e_end = a.e_end;
    int64_t grid[dev::BLOCKS_KINDS];
    grid[dev::BLOCKS_DOT] = dot_grid(ctx, Q, max_parts);
    grid[dev::BLOCKS_PARTS] = block_size ? std::max<int64_t>(1, std::min<int64_t>((rows / block_size + 255) / 256, 2048)) : 1;
    grid[dev::BLOCKS_DIRECTION] = block_size ? std::max<int64_t>(1, std::min<int64_t>((rows + 255) / 256, 4096)) : 1;
    grid[dev::BLOCKS_APPLY] = apply_grid(ctx, Q);
    for (int k = 0; k < dev::BLOCKS_KINDS; ++k) {
      g.first[k] = int32_t(total[k]);
      g.grid[k] = int32_t(grid[k]);
      total[k] += grid[k];
    }
  }
}

void hdd::abi::apply_blocks_kernel_name(std::string& out, const ApplyPlan& P, bool dot)
{
  out += P.tile ? "apply_tile_blocks_kernel<" : "apply_csr_blocks_kernel<";
  out += P.tile ? (P.nb == 3 ? "3, 3" : "4, 4") : (P.short_rows ? "8" : "64");
  out += dot ? ", dot>" : ">";
}

int hdd::abi::run_apply_blocks(const char* who, hdd_ctx* ctx, const ApplyPlan& P, const dev::BlockSegment* d_tab, int32_t n_blocks,
                               int64_t grid, const double* d_x, double* d_y, void* stream)
{
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, who);
  dev::ApplyArgs a = P.a;
  a.nv = 1;
  a.x = d_x;
  a.y = d_y;
  a.ldx = a.ldy = P.rows();
  const dev::BlocksArgs B{d_tab, n_blocks, dev::BLOCKS_APPLY, P.a.row_begin, nullptr, nullptr};
  last_apply_kernel_slot().clear();
  apply_blocks_kernel_name(last_apply_kernel_slot(), P, false);
  e = launch_apply_blocks<false>(P, a, B, grid, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? HDD_OK : hip_fail(e, who);
}

extern "C" const char* hdd_last_apply_kernel(void) { return last_apply_kernel_slot().c_str(); }

namespace {
// hdd_operator_apply (per_vector false: theta is [n_comp]) and hdd_operator_apply_multi (theta is [n_vec][ldt])
int apply(const char* who, bool per_vector, hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
          int32_t n_comp, const double* theta, int64_t ldt, const hdd_block_range* range, const double* d_x, int64_t ldx,
          double* d_y, int64_t ldy, int32_t n_vec, void* stream)
{
  if (!d_x || !d_y) return fail(HDD_ERR_INVALID, who, "null argument");
  if (n_vec < 1 || n_vec > HDD_MAX_VEC) return fail(HDD_ERR_INVALID, who, "n_vec outside 1..HDD_MAX_VEC");
  ApplyPlan P;
  if (int rc = plan_apply(who, ctx, mesh, pattern, d_vals, n_comp, per_vector ? nullptr : theta, range, P, per_vector)) return rc;
  if (per_vector && theta && ldt < n_comp) return fail(HDD_ERR_INVALID, who, "ldt smaller than n_comp");
  if (ldx < P.a.col_end - P.a.col_begin || ldy < P.rows())
    return fail(HDD_ERR_INVALID, who, "ldx / ldy smaller than the range");
  const ApplyThetas T{theta, ldt};
  return run_apply(who, ctx, P, per_vector ? &T : nullptr, d_x, ldx, d_y, ldy, n_vec, stream);
}
}  // namespace

extern "C" int hdd_operator_apply_multi(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                                        int32_t n_comp, const double* theta, int64_t ldt, const hdd_block_range* range,
                                        const double* d_x, int64_t ldx, double* d_y, int64_t ldy, int32_t n_vec, void* stream)
{
  return apply("hdd_operator_apply_multi", true, ctx, mesh, pattern, d_vals, n_comp, theta, ldt, range, d_x, ldx, d_y, ldy, n_vec, stream);
}

extern "C" int hdd_operator_apply(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern,
                                  const double* const* d_vals, int32_t n_comp, const double* theta,
                                  const hdd_block_range* range, const double* d_x, int64_t ldx, double* d_y,
                                  int64_t ldy, int32_t n_vec, void* stream)
{
  return apply("hdd_operator_apply", false, ctx, mesh, pattern, d_vals, n_comp, theta, 0, range, d_x, ldx, d_y, ldy, n_vec, stream);
}

// The table goes through the context's pinned buffer into its device buffer (both as old as the context): the event
// says when the previous call's copy has read the pinned one.
extern "C" int hdd_operator_apply_blocks(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                                         int32_t n_comp, const double* theta, int32_t n_blocks, const int64_t* bounds,
                                         const double* d_x, double* d_y, void* stream)
{
  const char* who = "hdd_operator_apply_blocks";
  if (!d_x || !d_y) return fail(HDD_ERR_INVALID, who, "null argument");
  ApplyPlan P;
  if (int rc = hdd::abi::plan_blocks(who, ctx, mesh, pattern, d_vals, n_comp, theta, n_blocks, bounds, P)) return rc;
  if (!ctx->blocks_tab_h || !ctx->blocks_tab_d || !ctx->blocks_evt) return fail(HDD_ERR_INVALID, who, "context without its segment table");
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = hipEventSynchronize(ctx->blocks_evt);
  if (e != hipSuccess) return hip_fail(e, who);
  auto* tab = static_cast<dev::BlockSegment*>(ctx->blocks_tab_h);
  int64_t total[dev::BLOCKS_KINDS];
  hdd::abi::blocks_table(ctx, P, n_blocks, bounds, 0, dev::APPLY2_BLOCKS, tab, total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  e = hipMemcpyAsync(ctx->blocks_tab_d, tab, size_t(n_blocks) * sizeof(dev::BlockSegment), hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipEventRecord(ctx->blocks_evt, s);
  if (e != hipSuccess) return hip_fail(e, who);
  return hdd::abi::run_apply_blocks(who, ctx, P, static_cast<const dev::BlockSegment*>(ctx->blocks_tab_d), n_blocks,
                                    total[dev::BLOCKS_APPLY], d_x, d_y, stream);
}

extern "C" int hdd_operator_apply2(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern,
                                   const double* const* d_vals, int32_t n_comp, const double* theta,
                                   const hdd_block_range* range, const double* d_v, int64_t ldv, int32_t n_v,
                                   const double* d_u, int64_t ldu, int32_t n_u, double* d_work, int64_t ldw,
                                   double* d_out, void* stream)
{
  const char* who = "hdd_operator_apply2";
  if (!d_v || !d_u || !d_work || !d_out) return fail(HDD_ERR_INVALID, who, "null argument");
  if (n_v < 1 || n_v > HDD_MAX_VEC || n_u < 1 || n_u > HDD_MAX_VEC)
    return fail(HDD_ERR_INVALID, who, "n_v / n_u outside 1..HDD_MAX_VEC");
  ApplyPlan P;
  if (int rc = plan_apply(who, ctx, mesh, pattern, d_vals, n_comp, theta, range, P)) return rc;
  const int64_t rows = P.a.row_end - P.a.row_begin;
  if (ldu < P.a.col_end - P.a.col_begin || ldv < rows || ldw < rows)
    return fail(HDD_ERR_INVALID, who, "ldv / ldu / ldw smaller than the range");
  if (!ctx->apply2_ws) return fail(HDD_ERR_INVALID, who, "context without its reduction buffer");
  if (int rc = run_apply(who, ctx, P, nullptr, d_u, ldu, d_work, ldw, n_u, stream)) return rc;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int blocks = int(std::min<int64_t>(dev::APPLY2_BLOCKS, std::max<int64_t>(1, (rows + 1023) / 1024)));
  hipLaunchKernelGGL(dev::apply2_partial_kernel, dim3(blocks), dim3(256), 0, s, d_v, ldv, n_v, d_work, ldw, n_u, rows,
                     ctx->apply2_ws);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, who);
  hipLaunchKernelGGL(dev::apply2_final_kernel, dim3(1), dim3(64), 0, s, ctx->apply2_ws, blocks, n_v, n_u, d_out);
  e = hipGetLastError();
  return e == hipSuccess ? HDD_OK : hip_fail(e, who);
}
