// dune-hdd_amd/csrc/kernels/abi_project.hip -- C ABI: reduced-basis projection on the assembled value arrays
// (hdd_operator_project, hdd_operator_project_workspace, hdd_vectors_inner; kernels in project_kernels.hh): the
// G_q = V^T A_q U, V^T b_q and Gramians of a reduced-basis / LRBMS loop, every component in one pass.  The operator
// arguments are checked by plan_apply (apply_plan.hh), as hdd_operator_apply's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "apply_plan.hh"
#include "project_kernels.hh"

using hdd::abi::ApplyPlan;
using hdd::abi::fail;
namespace dev = hdd::dev;

namespace {
bool basis_size(int32_t n) { return n >= 1 && n <= HDD_MAX_BASIS; }

// Parts of a launch (= partial sums per entry): a function of the plan and the row count alone, never of the basis
// sizes.  Tile kernel: dot_grid's rule (tile_range wants a multiple of 8 below the tile count); CSR kernel: four
// waves of 32 (16) rows per workgroup pass.
int64_t project_parts(const hdd_ctx* ctx, const ApplyPlan& P)
{
  if (P.tile) return hdd::abi::dot_grid(ctx, P, dev::PROJECT_BLOCKS);
  const int64_t per_wg = 4 * dev::project_csr_rows(P.short_rows ? 8 : 64);
  return std::max<int64_t>(1, std::min<int64_t>((P.rows() + per_wg - 1) / per_wg, dev::PROJECT_BLOCKS));
}

int finish(const char* who, const double* d_work, int64_t parts, int64_t n_out, double* d_out, hipStream_t s)
{
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, who);
  hipLaunchKernelGGL(dev::project_final_kernel, dim3(unsigned((n_out + 255) / 256)), dim3(256), 0, s, d_work, int(parts), n_out, d_out);
  e = hipGetLastError();
  return e == hipSuccess ? HDD_OK : hip_fail(e, who);
}
}  // namespace

extern "C" int64_t hdd_operator_project_workspace(int32_t n_comp, int32_t n_v, int32_t n_u)
{
  if (n_comp < 1 || n_comp > HDD_MAX_COMP || !basis_size(n_v) || !basis_size(n_u)) return 0;
  return int64_t(dev::PROJECT_BLOCKS) * n_comp * n_v * n_u;
}

extern "C" int hdd_operator_project(hdd_ctx* ctx, const hdd_mesh* mesh, const hdd_csr* pattern, const double* const* d_vals,
                                    int32_t n_comp, const hdd_block_range* range, const double* d_v, int64_t ldv, int32_t n_v,
                                    const double* d_u, int64_t ldu, int32_t n_u, double* d_work, int64_t n_work, double* d_out,
                                    void* stream)
{
  const char* who = "hdd_operator_project";
  if (!d_v || !d_u || !d_work || !d_out) return fail(HDD_ERR_INVALID, who, "null argument");
  if (!basis_size(n_v) || !basis_size(n_u)) return fail(HDD_ERR_INVALID, who, "n_v / n_u outside 1..HDD_MAX_BASIS");
  ApplyPlan P;
  if (int rc = hdd::abi::plan_apply(who, ctx, mesh, pattern, d_vals, n_comp, nullptr, range, P)) return rc;
  if (ldv < P.rows() || ldu < P.a.col_end - P.a.col_begin) return fail(HDD_ERR_INVALID, who, "ldv / ldu smaller than the range");
  if (n_work < hdd_operator_project_workspace(n_comp, n_v, n_u))
    return fail(HDD_ERR_INVALID, who, "n_work below hdd_operator_project_workspace");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hdd::abi::name_project_kernel(P);
  dev::ProjectArgs pa;
  pa.a = P.a;
  pa.a.x = d_u;
  pa.a.ldx = ldu;
  pa.v = d_v;
  pa.ldv = ldv;
  pa.n_v = n_v;
  pa.n_u = n_u;
  pa.partial = d_work;
  const int n_panels = (n_u + dev::PROJECT_PANEL - 1) / dev::PROJECT_PANEL;
  const int64_t n_out = int64_t(n_comp) * n_v * n_u;
  int64_t parts = 0;   // no rows: the sum over no parts
  if (P.rows() > 0) {
    parts = project_parts(ctx, P);
    const dim3 g{unsigned(parts), unsigned(n_comp * n_panels)};
    if (P.tile && P.nb == 3)
      hipLaunchKernelGGL((dev::project_tile_kernel<3, 3>), g, dim3(64), (dev::ProjectTile<3, 3>::BYTES), s, pa, P.n_tiles(), n_panels);
    else if (P.tile)
      hipLaunchKernelGGL((dev::project_tile_kernel<4, 4>), g, dim3(64), (dev::ProjectTile<4, 4>::BYTES), s, pa, P.n_tiles(), n_panels);
    else if (P.short_rows)
      hipLaunchKernelGGL((dev::project_csr_kernel<8>), g, dim3(256), 0, s, pa, n_panels);
    else
      hipLaunchKernelGGL((dev::project_csr_kernel<64>), g, dim3(256), 0, s, pa, n_panels);
  }
  return finish(who, d_work, parts, n_out, d_out, s);
}

extern "C" int hdd_vectors_inner(hdd_ctx* ctx, const double* d_v, int64_t ldv, int32_t n_v, const double* d_w, int64_t ldw,
                                 int32_t n_w, int64_t n, double* d_work, int64_t n_work, double* d_out, void* stream)
{
  const char* who = "hdd_vectors_inner";
  if (!ctx || !d_v || !d_w || !d_work || !d_out) return fail(HDD_ERR_INVALID, who, "null argument");
  if (!basis_size(n_v) || !basis_size(n_w)) return fail(HDD_ERR_INVALID, who, "n_v / n_w outside 1..HDD_MAX_BASIS");
  if (n < 0) return fail(HDD_ERR_INVALID, who, "negative n");
  if (ldv < n || ldw < n) return fail(HDD_ERR_INVALID, who, "ldv / ldw smaller than n");
  if (n_work < hdd_operator_project_workspace(1, n_v, n_w))
    return fail(HDD_ERR_INVALID, who, "n_work below hdd_operator_project_workspace(1, n_v, n_w)");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t parts = 0;
  if (n > 0) {
    parts = std::min<int64_t>((n + 255) / 256, dev::PROJECT_BLOCKS);   // a function of n alone
    const dim3 g{unsigned(parts), unsigned((n_w + dev::PROJECT_PANEL - 1) / dev::PROJECT_PANEL)};
    hipLaunchKernelGGL(dev::inner_kernel, g, dim3(256), 0, s, d_v, ldv, n_v, d_w, ldw, n_w, n, d_work);
  }
  return finish(who, d_work, parts, int64_t(n_v) * n_w, d_out, s);
}
