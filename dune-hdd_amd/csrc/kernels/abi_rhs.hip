// dune-hdd_amd/csrc/kernels/abi_rhs.hip -- C ABI: right-hand side functionals and products (kernels: rhs.hip and
// products.hip; P1 / Q1 products with piecewise-constant data: the persistent tile driver)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "abi_common.hh"
#include "quadrature.hh"

using namespace hdd;
using namespace hdd::abi;

static dev::KappaArg kap_arg(const hdd_scalar_fn* f)
{
  if (!f) return dev::KappaArg{HDD_FN_CONST, 0, 0.0, 0.0, 0.0, 0.0, nullptr, nullptr, 0, 0};
  return dev::KappaArg{f->kind, f->order, f->c, f->b, f->kx, f->ky, f->per_elem, f->table, f->n_table, 0};
}

// the tensor fields of RhsArgs / ProductArgs
template <class Args>
static void set_tensor(Args& a, const hdd_tensor_fn* tensor)
{
  a.tkind = tensor ? tensor->kind : HDD_TENSOR_CONST;
  for (int r = 0; r < 6; ++r) a.tc[r] = tensor ? tensor->c[r] : 0.0;
  a.tper = tensor ? tensor->per_elem : nullptr;
}

// the 1D Gauss rule on [0, 1] that is exact to `order`: points into q[.][0], weights into q[.][wcol]; returns the
// number of points, -1 beyond 16
template <int W>
static int gauss_rule_1d(int order, double (*q)[W], int wcol)
{
  const int n1 = std::max(1, (order + 2) / 2);
  if (n1 > 16) return -1;
  double s[16], w[16];
  gauss_legendre01(n1, s, w);
  for (int k = 0; k < n1; ++k) { q[k][0] = s[k]; q[k][wcol] = w[k]; }
  return n1;
}

extern "C" int hdd_swipdg_rhs(hdd_ctx* ctx, const hdd_mesh* m, const hdd_scalar_fn* force, const hdd_scalar_fn* kappa,
                              const hdd_tensor_fn* tensor, const hdd_scalar_fn* dirichlet,
                              const hdd_scalar_fn* neumann, const hdd_swipdg_params* p, double* d_rhs, void* stream)
{
  using namespace hdd::dev;
  static const char* who = "hdd_swipdg_rhs";
  if (!ctx || !m || !p || !d_rhs) return fail(HDD_ERR_INVALID, who, "null argument");
  if (int rc = check_elem_type(who, m)) return rc;
  if (!m->coords || !m->neighbors) return fail(HDD_ERR_INVALID, who, "mesh arrays missing");
  if (int rc = check_own_range(who, m)) return rc;
  if (dirichlet && (!kappa || !tensor))
    return fail(HDD_ERR_INVALID, who, "the Dirichlet functional needs kappa and the tensor");
  for (const hdd_scalar_fn* f : {force, kappa, dirichlet, neumann}) {
    if (int rc = check_fn_per_elem(who, f)) return rc;
    // (on HDD_HEX a FLATTOP function without table storage has always been INVALID, with storage UNSUPPORTED)
    if (int rc = check_flattop(who, f, m->elem_type, HDD_ERR_INVALID,
                               f && !f->table ? HDD_ERR_INVALID : HDD_ERR_UNSUPPORTED))
      return rc;
  }
  if (int rc = check_tensor(who, tensor)) return rc;
  int deg = 1;
  if (int rc = check_degree(who, m, &deg)) return rc;
  const int dim = m->elem_type == HDD_HEX ? 3 : 2;
  RhsArgs a{};
  a.elem_type = m->elem_type;
  a.degree = deg;
  a.nb = mesh_nb(m->elem_type, deg);
  a.n_local = m->n_local;
  a.own_begin = m->own_begin;
  a.own_end = m->own_end;
  a.coords = m->coords;
  if (int rc = check_vertex_arrays(who, m)) return rc;
  if (use_vertex_geometry(ctx, m, /*simplex_only=*/false, /*offsets32=*/false)) {
    a.ev = m->elem_vertices;
    a.vxy = m->vertex_coords;
  }
  a.nbrs = m->neighbors;
  set_tensor(a, tensor);
  a.force = kap_arg(force);
  a.kappa = kap_arg(kappa);
  a.dirichlet = kap_arg(dirichlet);
  a.neumann = kap_arg(neumann);
  a.has_force = force != nullptr;
  a.has_dirichlet = dirichlet != nullptr;
  a.has_neumann = neumann != nullptr;
  a.sigma_boundary = p->sigma_boundary;
  a.beta = p->beta;
  a.out = d_rhs;
  a.n_cu = ctx->n_cu;
  a.generic = (ctx->variant & HDD_VARIANT_RHS_GENERIC) ? 1 : 0;
  a.no_tiny = (ctx->variant & HDD_VARIANT_RHS_NO_TINY) ? 1 : 0;
  if (force) {
    const int order = fn_order(*force) + deg;
    a.nqv = m->elem_type == HDD_SIMPLEX ? simplex_rule(order, a.qv, 64) : tensor_rule(dim, order, a.qv, 64);
    if (a.nqv < 0) return set_error(HDD_ERR_UNSUPPORTED, "hdd_swipdg_rhs: force integration order too high");
  }
  if (dirichlet) {
    const int order = std::max(fn_order(*dirichlet) + deg, fn_order(*kappa) + 0 + (deg - 1) + fn_order(*dirichlet));
    a.nqd = face_rule(dim - 1, order, a.qd, 16);
    if (a.nqd < 0) return set_error(HDD_ERR_UNSUPPORTED, "hdd_swipdg_rhs: Dirichlet integration order too high");
  }
  if (neumann) {
    a.nqn = face_rule(dim - 1, fn_order(*neumann) + deg, a.qn, 16);
    if (a.nqn < 0) return set_error(HDD_ERR_UNSUPPORTED, "hdd_swipdg_rhs: Neumann integration order too high");
  }
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_swipdg_rhs: hipSetDevice");
  const int64_t n_own = m->own_end - m->own_begin;
  // split path (HDD_VARIANT_RHS_FUSED: the fused kernel, cross-check): the list is kept in the context, allocated
  // (and its counters zeroed) on the first call of a size class -- warm up before hipGraph capture
  if (m->elem_type != HDD_HEX && (dirichlet || neumann) && n_own > 0 && n_own < (int64_t(1) << 31) &&
      !(ctx->variant & HDD_VARIANT_RHS_FUSED)) {
    const size_t bytes = hdd::dev::rhs_list_bytes(n_own);
    const bool grows = bytes > ctx->rhs_ws.bytes;
    // (any stream's earlier call may still read the old list: the whole device is waited for before it is freed)
    if ((e = ctx->rhs_ws.reserve(bytes, DeviceScratch::QUARTER, DeviceScratch::SYNC_DEVICE)) != hipSuccess)
      return hip_fail(e, "hdd_swipdg_rhs: list");
    if (grows && (e = hipMemset(ctx->rhs_ws.p, 0, RHS_LIST_OFS * sizeof(uint32_t))) != hipSuccess) {
      ctx->rhs_ws.release();   // (a list without zeroed counters must not be taken for warm)
      return hip_fail(e, "hdd_swipdg_rhs: list counters");
    }
    a.bnd_list = static_cast<uint32_t*>(ctx->rhs_ws.p);
  }
  a.skip_face = (ctx->debug_flags & 524288) ? 1 : 0;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  // The boundary-element list is context state: calls on different streams are ordered behind each other (the
  // previous call's face kernel has re-armed the counters before this call's volume kernel appends).  Not under
  // hipGraph capture, where the captured stream alone orders the replays.
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool ordered = a.bnd_list && hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
  if (ordered) {
    if (!ctx->rhs_evt && (e = hipEventCreateWithFlags(&ctx->rhs_evt, hipEventDisableTiming)) != hipSuccess)
      return hip_fail(e, "hdd_swipdg_rhs: list event");
    if (ctx->rhs_used && ctx->rhs_stream != s && (e = hipStreamWaitEvent(s, ctx->rhs_evt, 0)) != hipSuccess)
      return hip_fail(e, "hdd_swipdg_rhs: order behind the previous call's stream");
  }
  e = launch_rhs(a, s);
  if (ordered) {
    const hipError_t er = hipEventRecord(ctx->rhs_evt, s);
    if (er != hipSuccess && e == hipSuccess) e = er;
    ctx->rhs_stream = s;
    ctx->rhs_used = true;
  }
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_swipdg_rhs: launch");
}

extern "C" int hdd_product_assemble(hdd_ctx* ctx, const hdd_mesh* m, int32_t product, const hdd_scalar_fn* kappa,
                                    const hdd_tensor_fn* tensor, const hdd_swipdg_params* p, const hdd_csr* pattern,
                                    double* d_vals, void* stream)
{
  using namespace hdd::dev;
  static const char* who = "hdd_product_assemble";
  if (!ctx || !m || !p || !pattern || !d_vals || !pattern->elem_ptr) return fail(HDD_ERR_INVALID, who, "null argument");
  if (product < HDD_PRODUCT_L2 || product > HDD_PRODUCT_PENALTY) return fail(HDD_ERR_INVALID, who, "unknown product");
  if (int rc = check_elem_type(who, m)) return rc;
  if (int rc = check_own_range(who, m)) return rc;
  const bool needs_coeff = product == HDD_PRODUCT_ELLIPTIC || product == HDD_PRODUCT_PENALTY;
  if (needs_coeff && (!kappa || !tensor))
    return fail(HDD_ERR_INVALID, who, "elliptic / penalty products need kappa and the tensor");
  if (needs_coeff) {   // (the other products ignore kappa and the tensor)
    if (int rc = check_fn_per_elem(who, kappa)) return rc;
    if (int rc = check_flattop(who, kappa, m->elem_type, HDD_ERR_UNSUPPORTED, HDD_ERR_UNSUPPORTED)) return rc;
    if (int rc = check_tensor(who, tensor)) return rc;
  }
  int deg = 1;
  if (int rc = check_degree(who, m, &deg)) return rc;
  const int nb = mesh_nb(m->elem_type, deg);
  if (int rc = check_pattern_rows(who, pattern, nb, m)) return rc;
  // the element-local kinds write nb values per row, the penalty nb per row and (own + interior face) block: what the
  // host can tell from nnz alone (the penalty's block count per row lives in the device arrays)
  const int64_t nnz_local = int64_t(nb) * nb * (m->own_end - m->own_begin);
  if (product != HDD_PRODUCT_PENALTY && pattern->nnz != nnz_local)
    return fail(HDD_ERR_INVALID, who, "element-local products need the volume pattern (nnz = nb^2 * owned elements)");
  if (product == HDD_PRODUCT_PENALTY && pattern->nnz < nnz_local)
    return fail(HDD_ERR_INVALID, who, "penalty pattern smaller than its diagonal blocks");
  ProductArgs a{};
  a.elem_type = m->elem_type;
  a.degree = deg;
  a.nb = nb;
  a.kind = product;
  a.n_local = m->n_local;
  a.own_begin = m->own_begin;
  a.own_end = m->own_end;
  a.coords = m->coords;
  a.nbrs = m->neighbors;
  a.elem_ptr = pattern->elem_ptr;
  set_tensor(a, tensor);
  a.kappa = kap_arg(kappa);
  a.sigma_inner = p->sigma_inner;
  a.sigma_boundary = p->sigma_boundary;
  a.beta = p->beta;
  a.vals = d_vals;
  // integrand orders + over_integrate (= 2): test + ansatz order [+ kappa + A]; gradients count p - 1
  const int over = 2, ko = kappa ? fn_order(*kappa) : 0;
  if (product <= HDD_PRODUCT_ELLIPTIC) {
    int order = product == HDD_PRODUCT_L2 ? 2 * deg + over : 2 * (deg - 1) + over;
    if (product == HDD_PRODUCT_ELLIPTIC) order += ko;
    a.nqv = m->elem_type == HDD_SIMPLEX ? simplex_rule(order, a.qv, 64) : gauss_rule_1d(order, a.qv, 3);
    if (a.nqv < 0) return set_error(HDD_ERR_UNSUPPORTED, "hdd_product_assemble: integration order too high");
  } else {
    const int order = product == HDD_PRODUCT_BOUNDARY_L2 ? 2 * deg + over : ko + 2 * deg + over;
    a.nq1f = gauss_rule_1d(order, a.qf, 1);
    if (a.nq1f < 0) return set_error(HDD_ERR_UNSUPPORTED, "hdd_product_assemble: integration order too high");
  }
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_product_assemble: hipSetDevice");
  if (m->elem_type != HDD_HEX && m->face_info) {
    // P1 / Q1 with piecewise-constant data: closed forms on the persistent tile driver
    AssembleArgs f = mesh_args(ctx, m, pattern);
    set_coefficients(f, tensor, p);
    f.n_comp = 1;
    f.kappa[0] = a.kappa;
    f.vals[0] = d_vals;
    if (int rc = check_vertex_arrays(who, m)) return rc;
    if (use_vertex_geometry(ctx, m, /*simplex_only=*/true, /*offsets32=*/true)) {
      f.ev = m->elem_vertices;
      f.vxy = m->vertex_coords;
    }
    bool fast = false;
    e = launch_product_fast(f, product, static_cast<hipStream_t>(stream), &fast);
    if (fast) return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_product_assemble: launch");
  }
  e = launch_product(a, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? HDD_OK : hip_fail(e, "hdd_product_assemble: launch");
}
