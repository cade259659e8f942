// dune-hdd_amd/csrc/kernels/abi_estimate.hip -- C ABI: the ESV2007 a-posteriori error estimator of P1 SWIPDG and the
// OS2014 localized (per-segment) estimator of BlockSWIPDG (kernels: estimate.hip; host tables:
// csrc/host/estimator_tables.cpp)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <string>

#include "abi_common.hh"
#include "estimate_kernels.hh"
#include "quadrature.hh"

using namespace hdd;
using namespace hdd::abi;

struct hdd_estimator {
  int device = 0;
  int32_t residual_star = 0;
  int64_t n_local = 0, n_vertices = 0;
  int64_t* patch_ptr = nullptr;    // device [n_vertices + 1]
  int32_t* patch_dof = nullptr;    // device [3 n_local]
  uint8_t* vertex_bnd = nullptr;   // device [n_vertices]
  bool host_only = true;
  // hdd_estimator_set_segments: host geometry (kept from the creation), host tables, device copies
  std::vector<int32_t> elem_vertices;
  std::vector<double> vertex_coords;
  SegmentTables seg;
  int64_t n_segments = 0, n_chunks = 0;
  int64_t* seg_tab = nullptr;      // device [2][S + 1]: bounds, chunk prefix
  double* seg_diam = nullptr;      // device [S]
  void free_segments()
  {
    if (seg_tab) (void)hipFree(seg_tab);
    if (seg_diam) (void)hipFree(seg_diam);
    seg_tab = nullptr;
    seg_diam = nullptr;
    n_segments = n_chunks = 0;
    seg = SegmentTables();
  }
  ~hdd_estimator()
  {
    free_segments();
    if (patch_ptr) (void)hipFree(patch_ptr);
    if (patch_dof) (void)hipFree(patch_dof);
    if (vertex_bnd) (void)hipFree(vertex_bnd);
  }
};

namespace {
const char*& last_estimate_kernels_slot()
{
  thread_local const char* names = "";
  return names;
}

// doubles of the workspace: Oswald values (what follows them begins at oswald_doubles: 16-byte aligned), the partial
// sums of the four quantities, their totals
int64_t oswald_doubles(int64_t n_vertices) { return (n_vertices + 1) & ~int64_t(1); }
int64_t workspace_doubles(int64_t n_local, int64_t n_vertices)
{
  return oswald_doubles(n_vertices) + 4 * dev::estimate_workgroups(n_local) + 4;
}

// the block call's: Oswald values, [4][n_chunks] partials, the four totals, [4][S] segment values
int64_t blocks_workspace_doubles(const hdd_estimator* est)
{
  return oswald_doubles(est->n_vertices) + 4 * est->n_chunks + 4 + 4 * est->n_segments;
}

// theta of a role on the host: NULL -> fallback (NULL: all ones)
void resolve_theta(int32_t n_comp, const double* th, const double* fallback, double* out)
{
  for (int q = 0; q < n_comp; ++q) out[q] = th ? th[q] : (fallback ? fallback[q] : 1.0);
}

// alpha(mu, mu') = min_q theta_q(mu) / theta_q(mu'), gamma = max_q of the same ratio
void alpha_gamma(int32_t n_comp, const double* mu, const double* other, double* alpha, double* gamma)
{
  *alpha = *gamma = mu[0] / other[0];
  for (int q = 1; q < n_comp; ++q) {
    *alpha = std::min(*alpha, mu[q] / other[q]);
    *gamma = std::max(*gamma, mu[q] / other[q]);
  }
}

template <class T>
hipError_t upload(T** d, const std::vector<T>& h)
{
  hipError_t e = hipMalloc(reinterpret_cast<void**>(d), std::max<size_t>(h.size(), 1) * sizeof(T));
  if (e != hipSuccess) {
    *d = nullptr;
    return e;
  }
  return h.empty() ? hipSuccess : hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
}
}  // namespace

extern "C" int hdd_estimator_create(hdd_ctx* ctx, const hdd_local* l, hdd_estimator** out)
{
  static const char* who = "hdd_estimator_create";
  if (!l || !out) return fail(HDD_ERR_INVALID, who, "null argument");
  *out = nullptr;
  EstimatorTables t;
  if (int rc = estimator_tables(l, &t)) return rc;   // (the scope checks: before the first device call)
  hdd_estimator* est = new (std::nothrow) hdd_estimator;
  if (!est) return fail(HDD_ERR_NOMEM, who, "out of host memory");
  est->n_local = t.n_local;
  est->n_vertices = t.n_vertices;
  est->elem_vertices.swap(t.elem_vertices);
  est->vertex_coords.swap(t.vertex_coords);
  *out = est;
  if (!ctx) return HDD_OK;   // host-only: sizes, no device tables
  *out = nullptr;
  est->device = ctx->device;
  est->host_only = false;
  hipError_t e = hipSetDevice(ctx->device);
  if (e == hipSuccess) e = upload(&est->patch_ptr, t.patch_ptr);
  if (e == hipSuccess) e = upload(&est->patch_dof, t.patch_dof);
  if (e == hipSuccess) e = upload(&est->vertex_bnd, t.vertex_bnd);
  if (e != hipSuccess) {
    delete est;
    return hip_fail(e, "hdd_estimator_create: tables");
  }
  *out = est;
  return HDD_OK;
}

extern "C" void hdd_estimator_destroy(hdd_estimator* est) { delete est; }

extern "C" int hdd_estimator_set_residual_star(hdd_estimator* est, int32_t on)
{
  if (!est) return fail(HDD_ERR_INVALID, "hdd_estimator_set_residual_star", "null estimator");
  est->residual_star = on != 0;
  return HDD_OK;
}

extern "C" int64_t hdd_estimator_workspace(const hdd_estimator* est)
{
  return est ? workspace_doubles(est->n_local, est->n_vertices) : 0;
}

extern "C" const char* hdd_last_estimate_kernels(void) { return last_estimate_kernels_slot(); }

namespace {
// the argument checks both estimate calls share (every one of them before the first device call) and the kernel
// arguments they have in common; n_need: the workspace of the call
int check_and_fill(const char* who, hdd_ctx* ctx, const hdd_estimator* est, const hdd_mesh* m, const hdd_scalar_fn* kappa,
                   int32_t n_comp, const double* theta_mu, const double* theta_bar, const double* theta_hat,
                   const hdd_tensor_fn* tensor, const hdd_scalar_fn* force, const hdd_swipdg_params* p, const double* d_u,
                   double* d_work, int64_t n_work, int64_t n_need, const char* need_name, double* d_local, double* d_flux,
                   double* d_oswald, double* sums, dev::EstimateArgs& a)
{
  if (!ctx || !est || !m || !kappa || !tensor || !p || !d_u || !d_work || !sums)
    return fail(HDD_ERR_INVALID, who, "null argument");
  if (n_comp < 1 || n_comp > HDD_MAX_COMP) return fail(HDD_ERR_INVALID, who, "n_comp outside 1..HDD_MAX_COMP");
  if (m->elem_type != HDD_SIMPLEX) return fail(HDD_ERR_UNSUPPORTED, who, "2d simplex meshes only");
  if (m->degree > 1) return fail(HDD_ERR_UNSUPPORTED, who, "degree 1 (P1) only");
  if (m->own_begin != 0 || m->own_end != m->n_local)
    return fail(HDD_ERR_UNSUPPORTED, who, "whole-grid view only (own_begin == 0, own_end == n_local)");
  if (m->n_local != est->n_local) return fail(HDD_ERR_INVALID, who, "the mesh is not the estimator's (n_local differs)");
  if (!m->elem_vertices || !m->vertex_coords)
    return fail(HDD_ERR_INVALID, who, "the mesh must carry elem_vertices / vertex_coords");
  if (!m->neighbors || !m->face_info) return fail(HDD_ERR_INVALID, who, "mesh arrays missing");
  for (int q = 0; q < n_comp; ++q) {
    if (kappa[q].kind != HDD_FN_CONST && kappa[q].kind != HDD_FN_PER_ELEM)
      return fail(HDD_ERR_UNSUPPORTED, who, "diffusion factor components must be CONST or PER_ELEM");
    if (int rc = check_fn_per_elem(who, &kappa[q])) return rc;
  }
  if (int rc = check_tensor_kind(who, tensor)) return rc;
  if (int rc = check_tensor(who, tensor)) return rc;
  if (int rc = check_fn_per_elem(who, force)) return rc;
  if (int rc = check_flattop(who, force, m->elem_type, HDD_ERR_INVALID, HDD_ERR_UNSUPPORTED)) return rc;
  if (force && (force->kind < HDD_FN_CONST || force->kind > HDD_FN_FLATTOP))
    return fail(HDD_ERR_UNSUPPORTED, who, "unknown force kind");
  if (!(p->beta == p->beta)) return fail(HDD_ERR_INVALID, who, "beta is NaN");
  if (n_work < n_need) return fail(HDD_ERR_INVALID, who, need_name);

  a.n = m->n_local;
  a.n_vertices = est->n_vertices;
  a.ev = m->elem_vertices;
  a.vxy = m->vertex_coords;
  a.nbrs = m->neighbors;
  a.finfo = m->face_info;
  a.patch_ptr = est->patch_ptr;
  a.patch_dof = est->patch_dof;
  a.vertex_bnd = est->vertex_bnd;
  a.u = d_u;
  a.oswald = d_work;
  a.out_local = d_local;
  a.out_flux = d_flux;
  a.out_oswald = d_oswald;
  a.n_comp = n_comp;
  a.tkind = tensor->kind;
  for (int r = 0; r < 3; ++r) a.tc[r] = tensor->c[r];
  a.tper = tensor->per_elem;
  const double* bar = theta_bar ? theta_bar : theta_mu;
  const double* hat = theta_hat ? theta_hat : theta_mu;
  for (int q = 0; q < n_comp; ++q) {
    a.kper[q] = kappa[q].kind == HDD_FN_PER_ELEM ? kappa[q].per_elem : nullptr;
    a.kconst[q] = kappa[q].c;
    a.theta[0][q] = theta_mu ? theta_mu[q] : 1.0;
    a.theta[1][q] = bar ? bar[q] : 1.0;
    a.theta[2][q] = hat ? hat[q] : 1.0;
  }
  // a force that is constant on every element has f - P0 f = 0: no residual term
  // (with residual_star the difference to div t_h remains: every force, an absent one as f = 0, is integrated)
  a.residual_star = est->residual_star;
  a.has_force = a.residual_star || (force && force->kind != HDD_FN_CONST && force->kind != HDD_FN_PER_ELEM);
  if (a.has_force) {
    a.force = dev::KappaArg{HDD_FN_CONST, 0, 0.0, 0.0, 0.0, 0.0, nullptr, nullptr, 0, 0};
    if (force)
      a.force = dev::KappaArg{force->kind, force->order, force->c, force->b, force->kx, force->ky, force->per_elem,
                              force->table, force->n_table, 0};
    const int order = force ? fn_order(*force) : 0;
    double q[64][4];
    for (int pass = 0; pass < 2; ++pass) {
      const int nq = simplex_rule(pass == 0 ? order + 2 : 2 * order + 2, q, 64);
      const int at = pass == 0 ? 0 : a.nqa;
      if (nq < 0 || at + nq > dev::ESTIMATE_QMAX)
        return fail(HDD_ERR_UNSUPPORTED, who, "force integration order too high");
      for (int k = 0; k < nq; ++k) {
        a.q[at + k][0] = q[k][0];
        a.q[at + k][1] = q[k][1];
        a.q[at + k][2] = q[k][3];
      }
      (pass == 0 ? a.nqa : a.nqb) = nq;
    }
  }
  a.sigma_inner = p->sigma_inner;
  a.sigma_boundary = p->sigma_boundary;
  a.beta = p->beta;
  a.beta_is_one = p->beta == 1.0;

  return HDD_OK;
}

// the end of both estimate calls, a filled: the checks that need the device tables, the launches (block: the OS2014
// call's), then the four totals come back through the context's pinned bytes (one synchronisation)
int launch_and_fetch(const char* who, hdd_ctx* ctx, const hdd_estimator* est, const dev::EstimateArgs& a, bool block, void* stream, double* sums)
{
  auto at = [who](const char* step) { return std::string(who) + step; };
  if (!est->patch_ptr || (block && !est->seg_tab))
    return fail(HDD_ERR_INVALID, who, "host-only estimator (created without a context)");
  if (!ctx->solve_state_h) return fail(HDD_ERR_INVALID, who, "context without its state buffer");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, at(": hipSetDevice").c_str());
  const hipStream_t s = static_cast<hipStream_t>(stream);
  e = block ? dev::launch_estimate_blocks(a, s, &last_estimate_kernels_slot()) : dev::launch_estimate(a, s, &last_estimate_kernels_slot());
  if (e != hipSuccess) return hip_fail(e, at(": launch").c_str());
  e = hipMemcpyAsync(ctx->solve_state_h, a.total, 4 * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, at(": sums").c_str());
  for (int r = 0; r < 4; ++r) sums[r] = ctx->solve_state_h[r];
  return HDD_OK;
}
}  // namespace

extern "C" int hdd_swipdg_estimate(hdd_ctx* ctx, const hdd_estimator* est, const hdd_mesh* m, const hdd_scalar_fn* kappa,
                                   int32_t n_comp, const double* theta_mu, const double* theta_bar,
                                   const double* theta_hat, const hdd_tensor_fn* tensor, const hdd_scalar_fn* force,
                                   const hdd_swipdg_params* p, const double* d_u, double* d_work, int64_t n_work,
                                   double* d_local, double* d_flux, double* d_oswald, double* sums, void* stream)
{
  static const char* who = "hdd_swipdg_estimate";
  dev::EstimateArgs a{};
  if (int rc = check_and_fill(who, ctx, est, m, kappa, n_comp, theta_mu, theta_bar, theta_hat, tensor, force, p, d_u, d_work,
                              n_work, est ? workspace_doubles(est->n_local, est->n_vertices) : 0,
                              "n_work below hdd_estimator_workspace", d_local, d_flux, d_oswald, sums, a))
    return rc;
  a.partial = d_work + oswald_doubles(est->n_vertices);
  a.total = a.partial + 4 * dev::estimate_workgroups(a.n);
  return launch_and_fetch(who, ctx, est, a, false, stream, sums);
}

extern "C" int hdd_estimator_set_segments(hdd_estimator* est, int64_t n_segments, const int64_t* bounds)
{
  static const char* who = "hdd_estimator_set_segments";
  if (!est) return fail(HDD_ERR_INVALID, who, "null estimator");
  if (n_segments == 0) {
    if (!est->host_only) {
      const hipError_t e = hipSetDevice(est->device);
      if (e != hipSuccess) return hip_fail(e, "hdd_estimator_set_segments: hipSetDevice");
    }
    est->free_segments();
    return HDD_OK;
  }
  SegmentTables t;
  if (int rc = estimator_segment_tables(est->n_local, est->n_vertices, est->elem_vertices.data(), est->vertex_coords.data(),
                                        n_segments, bounds, &t))
    return rc;   // (the tables of the last valid call stay)
  int64_t* tab = nullptr;
  double* diam = nullptr;
  if (!est->host_only) {
    hipError_t e = hipSetDevice(est->device);
    std::vector<int64_t> both(t.bounds);
    both.insert(both.end(), t.chunk_prefix.begin(), t.chunk_prefix.end());
    if (e == hipSuccess) e = upload(&tab, both);
    if (e == hipSuccess) e = upload(&diam, t.diam);
    if (e != hipSuccess) {
      if (tab) (void)hipFree(tab);
      if (diam) (void)hipFree(diam);
      return hip_fail(e, "hdd_estimator_set_segments: tables");
    }
  }
  est->free_segments();
  est->seg.bounds.swap(t.bounds);
  est->seg.chunk_prefix.swap(t.chunk_prefix);
  est->seg.diam.swap(t.diam);
  est->n_segments = n_segments;
  est->n_chunks = est->seg.chunk_prefix[size_t(n_segments)];
  est->seg_tab = tab;
  est->seg_diam = diam;
  return HDD_OK;
}

extern "C" int hdd_estimator_segment_diameters(const hdd_estimator* est, double* out)
{
  static const char* who = "hdd_estimator_segment_diameters";
  if (!est || !out) return fail(HDD_ERR_INVALID, who, "null argument");
  if (est->n_segments == 0) return fail(HDD_ERR_INVALID, who, "no segments set (hdd_estimator_set_segments)");
  std::copy(est->seg.diam.begin(), est->seg.diam.end(), out);
  return HDD_OK;
}

extern "C" int64_t hdd_estimator_blocks_workspace(const hdd_estimator* est)
{
  return est && est->n_segments > 0 ? blocks_workspace_doubles(est) : 0;
}

extern "C" int hdd_os2014_factors(int32_t n_comp, const double* theta_mu, const double* theta_bar, const double* theta_hat,
                                  double out[5])
{
  static const char* who = "hdd_os2014_factors";
  if (!out) return fail(HDD_ERR_INVALID, who, "null argument");
  if (n_comp < 1 || n_comp > HDD_MAX_COMP) return fail(HDD_ERR_INVALID, who, "n_comp outside 1..HDD_MAX_COMP");
  double th[3][HDD_MAX_COMP];
  resolve_theta(n_comp, theta_mu, nullptr, th[0]);
  resolve_theta(n_comp, theta_bar, theta_mu, th[1]);
  resolve_theta(n_comp, theta_hat, theta_mu, th[2]);
  for (int r = 0; r < 3; ++r)
    if (!theta_positive(n_comp, th[r])) return fail(HDD_ERR_INVALID, who, "a theta component is not positive");
  alpha_gamma(n_comp, th[0], th[1], &out[0], &out[1]);
  alpha_gamma(n_comp, th[0], th[2], &out[2], &out[3]);
  out[4] = std::max(std::sqrt(out[3]), 1.0 / std::sqrt(out[2]));
  return HDD_OK;
}

extern "C" int hdd_block_swipdg_estimate(hdd_ctx* ctx, const hdd_estimator* est, const hdd_mesh* m,
                                         const hdd_scalar_fn* kappa, int32_t n_comp, const double* theta_mu,
                                         const double* theta_bar, const double* theta_hat, const double* theta_min,
                                         const double* theta_max, const hdd_tensor_fn* tensor, const hdd_scalar_fn* force,
                                         const hdd_swipdg_params* p, const double* d_u, double* d_work, int64_t n_work,
                                         double* d_local, double* d_flux, double* d_oswald, double* d_segments,
                                         double* sums, void* stream)
{
  static const char* who = "hdd_block_swipdg_estimate";
  if (est && est->n_segments == 0) return fail(HDD_ERR_INVALID, who, "no segments set (hdd_estimator_set_segments)");
  dev::EstimateArgs a{};
  if (int rc = check_and_fill(who, ctx, est, m, kappa, n_comp, theta_mu, theta_bar, theta_hat, tensor, force, p, d_u, d_work,
                              n_work, est ? blocks_workspace_doubles(est) : 0,
                              "n_work below hdd_estimator_blocks_workspace", d_local, d_flux, d_oswald, sums, a))
    return rc;
  resolve_theta(n_comp, theta_min, theta_mu, a.theta[3]);
  resolve_theta(n_comp, theta_max, theta_mu, a.theta[4]);
  for (int r = 0; r < 5; ++r)
    if (!theta_positive(n_comp, a.theta[r]))
      return fail(HDD_ERR_INVALID, who, "a theta component is not positive (mu, mu_bar, mu_hat, mu_min, mu_max)");
  double f[5];
  if (int rc = hdd_os2014_factors(n_comp, a.theta[0], a.theta[1], a.theta[2], f)) return rc;
  a.factor[0] = std::sqrt(f[1]);
  a.factor[1] = f[4];
  a.factor[2] = 1.0 / std::sqrt(f[0]);
  const int64_t S = est->n_segments;
  a.n_segments = S;
  a.n_chunks = est->n_chunks;
  a.seg_bounds = est->seg_tab;
  a.chunk_prefix = est->seg_tab + (S + 1);
  a.seg_diam = est->seg_diam;
  a.partial = d_work + oswald_doubles(est->n_vertices);
  a.total = a.partial + 4 * a.n_chunks;
  a.segments = d_segments ? d_segments : a.total + 4;
  return launch_and_fetch(who, ctx, est, a, true, stream, sums);
}
