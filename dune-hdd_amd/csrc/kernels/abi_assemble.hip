// dune-hdd_amd/csrc/kernels/abi_assemble.hip -- C ABI: SWIPDG assembly dispatch (2d tile driver and HDD_HEX) and the
// sharded step's fixup entry points (hdd_internal.hh, used by shard_step.hip)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "abi_common.hh"
#include "quadrature.hh"

using hdd::set_error;
using namespace hdd::abi;

namespace {
const char* const WHO = "hdd_swipdg_assemble";

// What a call of assemble_impl covers and where its values go: every tile (list == nullptr), the listed tiles, or
// the listed elements in one of the element-pass forms (AssembleArgs::list_elements)
struct AssembleMode {
  const int32_t* list = nullptr;   // tiles or owned elements, relative to own_begin
  int64_t n_list = 0;
  int32_t list_kind = hdd::dev::LIST_TILES;
  bool skip_ghost = false;         // tiles leave the row blocks of elements with a ghost face neighbour alone
  int32_t reserve_wg = 0;          // full-range launches: workgroup slots left to a concurrent element pass
  int64_t fix_ld = 0;              // LIST_SIDE_SOA: leading dimension of the side buffers
};
}  // namespace

// ---------------------------------------------------------------------------------------------------
// HDD_HEX: Q_p on affine hexahedra (hex_qp.hip)
// ---------------------------------------------------------------------------------------------------
static int assemble_hex(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                        const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                        double* const* d_vals, void* stream)
{
  using namespace hdd::dev;
  int deg = 1;
  if (int rc = check_degree(WHO, m, &deg)) return rc;
  if (int rc = check_pattern_rows(WHO, pattern, mesh_nb(HDD_HEX, deg), m)) return rc;
  if (int rc = check_tensor_kind(WHO, tensor)) return rc;
  if (int rc = check_tensor(WHO, tensor)) return rc;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_swipdg_assemble: hipSetDevice");
  for (int c = 0; c < n_comp; ++c) {
    const hdd_scalar_fn& k = kappa[c];
    if (k.kind != HDD_FN_CONST && k.kind != HDD_FN_PER_ELEM && k.kind != HDD_FN_SINUSOID)
      return fail(HDD_ERR_UNSUPPORTED, WHO, "unknown diffusion factor kind");
    if (int rc = check_fn_per_elem(WHO, &k)) return rc;
    if (!d_vals[c]) return fail(HDD_ERR_INVALID, WHO, "null value array");
    // integrand orders (dune-gdt): volume ord(kappa) + ord(A) + 2 (p-1), faces ord(kappa) + ord(A) + 2p
    const int ko = fn_order(k);
    const int vol_order = p->vol_order >= 0 ? p->vol_order : ko + 2 * (deg - 1);
    const int face_order = p->face_order >= 0 ? p->face_order : ko + 2 * deg;
    const int nq1v = std::max(1, (vol_order + 2) / 2), nq1f = std::max(1, (face_order + 2) / 2);
    if (nq1v > 8 || nq1f > 8) return fail(HDD_ERR_UNSUPPORTED, WHO, "quadrature order too high for HDD_HEX");
    HexArgs a{};
    a.n_local = m->n_local;
    a.own_begin = m->own_begin;
    a.own_end = m->own_end;
    a.coords = m->coords;
    a.nbrs = m->neighbors;
    a.elem_ptr = pattern->elem_ptr;
    a.tkind = tensor->kind;
    for (int r = 0; r < 6; ++r) a.tc[r] = tensor->c[r];
    a.tper = tensor->per_elem;
    a.kkind = k.kind;
    a.kc = k.c;
    a.kb = k.b;
    a.kx = k.kx;
    a.ky = k.ky;
    a.kper = k.per_elem;
    a.vals = d_vals[c];
    a.sigma_inner = p->sigma_inner;
    a.sigma_boundary = p->sigma_boundary;
    a.beta = p->beta;
    a.debug_flags = ctx->debug_flags;   // profiling ablations (HDD_ABLATION builds only)
    a.variant = ctx->variant;
    HexTables& t = a.tab;
    hdd::hex_tables(deg, nq1v, nq1f, {t.sv, t.wv, t.sf, t.wf, t.Lv, t.Dv, t.Lf, t.Df, t.Le, t.De});
    if (hex_uses_records(a, deg, nq1v, nq1f)) {
      const int64_t n_own = std::max<int64_t>(1, m->own_end - m->own_begin);
      e = ctx->ws.reserve(hex_q3_workspace_doubles(n_own) * sizeof(double), DeviceScratch::QUARTER,
                          DeviceScratch::NO_SYNC);
      if (e != hipSuccess) return hip_fail(e, "hdd_swipdg_assemble: workspace");
      a.ws = static_cast<double*>(ctx->ws.p);
      a.q3g_coef = a.ws + n_own * HEX_REC;
      a.q3g_meta = reinterpret_cast<int64_t*>(a.q3g_coef + (n_own + 15) / 16 * 16 * Q3G_K);
      if (!ctx->q3g_tab) {   // element-independent: the 1D tables are fixed for (p, nq1v, nq1f) = (3, 3, 4)
        std::vector<double> tab(size_t(Q3G_K) * 4096);
        hex_q3g_reference_tables(a.tab, tab.data());
        e = hipMalloc(&ctx->q3g_tab, tab.size() * sizeof(double));
        if (e != hipSuccess) return hip_fail(e, "hdd_swipdg_assemble: reference matrices");
        e = hipMemcpy(ctx->q3g_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "hdd_swipdg_assemble: reference matrices");
      }
      a.q3g_tab = ctx->q3g_tab;
      // 4 row waves per workgroup, 128 workgroups per replica: 2 replicas per 128 CUs (8 waves per CU)
      a.q3g_reps = ctx->q3g_reps > 0 ? ctx->q3g_reps : std::max(1, ctx->n_cu / 64);
    }
    bool supported = false;
    e = launch_hex(a, deg, nq1v, nq1f, static_cast<hipStream_t>(stream), &supported);
    if (!supported)
      return set_error(HDD_ERR_UNSUPPORTED, "hdd_swipdg_assemble: no HDD_HEX kernel for p=" + std::to_string(deg) +
                                                ", volume order " + std::to_string(vol_order) + ", face order " +
                                                std::to_string(face_order));
    if (e != hipSuccess) return hip_fail(e, "hdd_swipdg_assemble: launch");
  }
  return HDD_OK;
}

static int assemble_impl(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                         const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                         double* const* d_vals, const AssembleMode& mode, void* stream)
{
  using namespace hdd::dev;
  if (!ctx || !m || !kappa || !tensor || !p || !pattern || !d_vals) return fail(HDD_ERR_INVALID, WHO, "null argument");
  if (n_comp < 1 || n_comp > HDD_MAX_COMP) return fail(HDD_ERR_INVALID, WHO, "need 1 <= n_comp <= HDD_MAX_COMP");
  if (int rc = check_elem_type(WHO, m)) return rc;
  if (!m->coords || !m->neighbors || !m->face_info || !pattern->elem_ptr)
    return fail(HDD_ERR_INVALID, WHO, "mesh / pattern arrays missing");
  if (int rc = check_own_range(WHO, m)) return rc;
  if (m->n_local >= int64_t(INT32_MAX)) return fail(HDD_ERR_RANGE, WHO, "n_local must fit int32 neighbour ids");
  // hdd_last_tile_kernel names the kernel THIS call launches (every launch path sets it); an element-list pass (the
  // sharded step's side pass beside its tile launch) leaves the tile launch's name in place
  if (mode.list_kind == LIST_TILES) hdd::last_tile_kernel_slot() = "";
  // The sharded step (shard_step.hip) runs this function on two streams at once with one context: the element-list
  // pass on the transfer stream beside the SKIP launch on the caller's stream.  That is safe only because the
  // 2d paths below (tiles, element lists, skip_ghost) use no context workspace (ws / scan_ws / rhs_ws); the
  // one path that does (HDD_HEX, p = 3) takes no lists, and the sharded step runs it exchange-then-assemble.
  if (m->elem_type == HDD_HEX) {
    if (mode.list || mode.skip_ghost)
      return set_error(HDD_ERR_UNSUPPORTED, "hdd_swipdg_assemble_tiles: no tile / element lists for HDD_HEX");
    return assemble_hex(ctx, m, kappa, n_comp, tensor, p, pattern, d_vals, stream);
  }
  int deg = 1;
  if (int rc = check_degree(WHO, m, &deg)) return rc;
  if (int rc = check_pattern_rows(WHO, pattern, mesh_nb(m->elem_type, deg), m)) return rc;
  if (int rc = check_tensor_kind(WHO, tensor)) return rc;
  if (int rc = check_tensor(WHO, tensor)) return rc;
  AssembleArgs a = mesh_args(ctx, m, pattern);
  set_coefficients(a, tensor, p);
  a.n_comp = n_comp;
  a.tile_list = mode.list;
  a.n_tile_list = mode.n_list;
  a.list_elements = mode.list_kind;
  a.skip_ghost = mode.skip_ghost ? 1 : 0;
  a.reserve_wg = mode.list_kind != LIST_TILES ? 0 : mode.reserve_wg;
  a.fix_ld = mode.fix_ld;
  a.fix_rb = hdd_fix_rb(m->elem_type);
  if (int rc = check_vertex_arrays(WHO, m)) return rc;
  if (use_vertex_geometry(ctx, m, /*simplex_only=*/false, /*offsets32=*/true)) {
    a.ev = m->elem_vertices;
    a.vxy = m->vertex_coords;
  }
  // integrand orders of LocalEvaluation::Elliptic / SWIPDG::Inner / BoundaryLHS at p = 1 (piecewise
  // constant tensors): volume ord(kappa); faces ord(kappa) + 2.  One kernel serves components of equal
  // order -- the caller splits mixed-order component sets.
  const int ko = fn_order(kappa[0]);
  for (int c = 0; c < n_comp; ++c) {
    const hdd_scalar_fn& k = kappa[c];
    if (k.kind != HDD_FN_CONST && k.kind != HDD_FN_PER_ELEM && k.kind != HDD_FN_SINUSOID && k.kind != HDD_FN_FLATTOP)
      return fail(HDD_ERR_UNSUPPORTED, WHO, "unknown diffusion factor kind");
    if (int rc = check_fn_per_elem(WHO, &k)) return rc;
    if (fn_order(k) != ko) return fail(HDD_ERR_UNSUPPORTED, WHO, "components of different integration order");
    if (!d_vals[c]) return fail(HDD_ERR_INVALID, WHO, "null value array");
    if (int rc = check_flattop(WHO, &k, m->elem_type, HDD_ERR_INVALID, HDD_ERR_UNSUPPORTED)) return rc;
    a.kappa[c] = KappaArg{k.kind, k.order, k.c, k.b, k.kx, k.ky, k.per_elem, k.table, k.n_table, 0};
    a.vals[c] = d_vals[c];
  }
  const int vol_order = p->vol_order >= 0 ? p->vol_order : ko;
  const int face_order = p->face_order >= 0 ? p->face_order : ko + 2;
  const int nqv = volume_points(m->elem_type, vol_order);
  const int nqf = face_points(face_order);
  bool supported = false;
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_swipdg_assemble: hipSetDevice");
  e = launch_assemble(a, nqv, nqf, static_cast<hipStream_t>(stream), &supported);
  if (!supported)
    return set_error(HDD_ERR_UNSUPPORTED, "hdd_swipdg_assemble: no kernel for volume order " + std::to_string(vol_order) +
                                              " / face order " + std::to_string(face_order));
  if (e != hipSuccess) return hip_fail(e, "hdd_swipdg_assemble: launch");
  return HDD_OK;
}

extern "C" int hdd_swipdg_assemble(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                                   const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                                   double* const* d_vals, void* stream)
{
  return assemble_impl(ctx, m, kappa, n_comp, tensor, p, pattern, d_vals, AssembleMode{}, stream);
}

extern "C" int hdd_swipdg_assemble_tiles(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                                         const hdd_tensor_fn* tensor, const hdd_swipdg_params* p,
                                         const hdd_csr* pattern, double* const* d_vals, const int32_t* d_tiles,
                                         int64_t n_tiles, void* stream)
{
  if (!d_tiles && n_tiles) return set_error(HDD_ERR_INVALID, "hdd_swipdg_assemble_tiles: null tile list");
  if (n_tiles == 0) return HDD_OK;
  AssembleMode mode;
  mode.list = d_tiles;
  mode.n_list = n_tiles;
  return assemble_impl(ctx, m, kappa, n_comp, tensor, p, pattern, d_vals, mode, stream);
}

// an element-list pass of the given form (AssembleArgs::list_elements)
static AssembleMode element_pass(int32_t list_kind, const int32_t* d_elems, int64_t n_elems)
{
  AssembleMode mode;
  mode.list = d_elems;
  mode.n_list = n_elems;
  mode.list_kind = list_kind;
  return mode;
}

extern "C" int hdd_swipdg_assemble_elements(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa,
                                            int32_t n_comp, const hdd_tensor_fn* tensor, const hdd_swipdg_params* p,
                                            const hdd_csr* pattern, double* const* d_vals, const int32_t* d_elems,
                                            int64_t n_elems, void* stream)
{
  if (!d_elems && n_elems) return set_error(HDD_ERR_INVALID, "hdd_swipdg_assemble_elements: null element list");
  if (n_elems == 0) return HDD_OK;
  return assemble_impl(ctx, m, kappa, n_comp, tensor, p, pattern, d_vals,
                       element_pass(hdd::dev::LIST_ELEMENTS, d_elems, n_elems), stream);
}

// ------------------------------------------------------------------------------------------------
// Sharded-step fixup off the assembly stream (shard_step.hip): the element-list pass writes each listed element's row
// block into a side buffer (slot fix_rb(m) doubles, one buffer of n + 1 slots per component) on the transfer
// stream while the full-range assembly runs; after the join, fix_scatter_kernel copies the blocks into place.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) fix_scatter_kernel(const double* __restrict__ buf, int32_t rb,
                                                         const int32_t* __restrict__ list, int64_t n,
                                                         const int64_t* __restrict__ elem_ptr, double* vals)
{
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t el = list[i];
    const int64_t b = elem_ptr[el], len = elem_ptr[el + 1] - b;
    for (int64_t k = threadIdx.x; k < len; k += 64) vals[b + k] = buf[i * rb + k];
  }
}

int hdd_fix_rb(int32_t elem_type) { return elem_type == HDD_SIMPLEX ? 3 * 3 * 4 : 4 * 4 * 5; }

int hdd_assemble_elements_buf(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                              const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                              double* const* d_bufs, const int32_t* d_elems, int64_t n_elems, void* stream)
{
  if (n_elems == 0) return HDD_OK;
  return assemble_impl(ctx, m, kappa, n_comp, tensor, p, pattern, d_bufs,
                       element_pass(hdd::dev::LIST_SIDE_BUFFER, d_elems, n_elems), stream);
}

int hdd_assemble_elements_inplace(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                                  const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                                  double* const* d_vals, const int32_t* d_elems, int64_t n_elems, void* stream)
{
  if (n_elems == 0) return HDD_OK;
  return assemble_impl(ctx, m, kappa, n_comp, tensor, p, pattern, d_vals,
                       element_pass(hdd::dev::LIST_IN_PLACE, d_elems, n_elems), stream);
}

int hdd_assemble_elements_soa(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                              const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                              double* const* d_bufs, int64_t ld, const int32_t* d_elems, int64_t n_elems, void* stream)
{
  if (n_elems == 0) return HDD_OK;
  if (m->elem_type != HDD_CUBE) return set_error(HDD_ERR_UNSUPPORTED, "hdd_assemble_elements_soa: Q1 only");
  AssembleMode mode = element_pass(hdd::dev::LIST_SIDE_SOA, d_elems, n_elems);
  mode.fix_ld = ld;
  return assemble_impl(ctx, m, kappa, n_comp, tensor, p, pattern, d_bufs, mode, stream);
}

int hdd_assemble_reserve(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                         const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                         double* const* d_vals, void* stream, int32_t reserve_wg)
{
  AssembleMode mode;
  mode.reserve_wg = reserve_wg;
  return assemble_impl(ctx, m, kappa, n_comp, tensor, p, pattern, d_vals, mode, stream);
}

int hdd_scatter_fix_q1_soa(hdd_ctx* ctx, const hdd_mesh* m, const hdd_csr* pattern, double* const* d_bufs, int64_t ld,
                           int32_t n_comp, const int32_t* d_elems, int64_t n_elems, double* const* d_vals, void* stream)
{
  if (n_elems == 0) return HDD_OK;
  hdd::dev::AssembleArgs a = mesh_args(ctx, m, pattern);
  a.tile_list = d_elems;
  a.n_tile_list = n_elems;
  for (int32_t c = 0; c < n_comp; ++c) {
    const hipError_t e = hdd::dev::launch_q1_scatter_soa(a, d_bufs[c], ld, d_vals[c], static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(e, "hdd_scatter_fix_q1_soa");
  }
  return HDD_OK;
}

int hdd_assemble_skip_ghost(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* kappa, int32_t n_comp,
                            const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                            double* const* d_vals, void* stream, int32_t reserve_wg)
{
  AssembleMode mode;
  mode.skip_ghost = true;
  mode.reserve_wg = reserve_wg;
  return assemble_impl(ctx, m, kappa, n_comp, tensor, p, pattern, d_vals, mode, stream);
}

int hdd_scatter_fix(hdd_ctx* ctx, const hdd_csr* pattern, int32_t rb, double* const* d_bufs, int32_t n_comp,
                    const int32_t* d_elems, int64_t n_elems, double* const* d_vals, void* stream)
{
  if (n_elems == 0) return HDD_OK;
  const unsigned grid = unsigned(std::min<int64_t>(n_elems, int64_t(ctx->n_cu) * 8));
  for (int32_t c = 0; c < n_comp; ++c) {
    hipLaunchKernelGGL(fix_scatter_kernel, dim3(grid), dim3(64), 0, static_cast<hipStream_t>(stream), d_bufs[c], rb,
                       d_elems, n_elems, pattern->elem_ptr, d_vals[c]);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "hdd_scatter_fix");
  }
  return HDD_OK;
}
