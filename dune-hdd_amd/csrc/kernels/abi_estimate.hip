// dune-hdd_amd/csrc/kernels/abi_estimate.hip -- C ABI: the ESV2007 a-posteriori error estimator of P1 SWIPDG (kernels:
// estimate.hip; host tables: csrc/host/estimator_tables.cpp)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>

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
  ~hdd_estimator()
  {
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

// doubles of the workspace: Oswald values, the partial sums of the four quantities, their totals (16-byte aligned parts)
int64_t workspace_doubles(int64_t n_local, int64_t n_vertices)
{
  return ((n_vertices + 1) & ~int64_t(1)) + 4 * dev::estimate_workgroups(n_local) + 4;
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
  *out = est;
  if (!ctx) return HDD_OK;   // host-only: sizes, no device tables
  *out = nullptr;
  est->device = ctx->device;
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

extern "C" int hdd_swipdg_estimate(hdd_ctx* ctx, const hdd_estimator* est, const hdd_mesh* m, const hdd_scalar_fn* kappa,
                                   int32_t n_comp, const double* theta_mu, const double* theta_bar,
                                   const double* theta_hat, const hdd_tensor_fn* tensor, const hdd_scalar_fn* force,
                                   const hdd_swipdg_params* p, const double* d_u, double* d_work, int64_t n_work,
                                   double* d_local, double* d_flux, double* d_oswald, double* sums, void* stream)
{
  static const char* who = "hdd_swipdg_estimate";
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
  if (n_work < workspace_doubles(est->n_local, est->n_vertices))
    return fail(HDD_ERR_INVALID, who, "n_work below hdd_estimator_workspace");

  dev::EstimateArgs a{};
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
  a.partial = d_work + ((est->n_vertices + 1) & ~int64_t(1));
  a.total = a.partial + 4 * dev::estimate_workgroups(a.n);
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

  if (!est->patch_ptr) return fail(HDD_ERR_INVALID, who, "host-only estimator (created without a context)");
  if (!ctx->solve_state_h) return fail(HDD_ERR_INVALID, who, "context without its state buffer");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return hip_fail(e, "hdd_swipdg_estimate: hipSetDevice");
  const hipStream_t s = static_cast<hipStream_t>(stream);
  e = dev::launch_estimate(a, s, &last_estimate_kernels_slot());
  if (e != hipSuccess) return hip_fail(e, "hdd_swipdg_estimate: launch");
  e = hipMemcpyAsync(ctx->solve_state_h, a.total, 4 * sizeof(double), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "hdd_swipdg_estimate: sums");
  for (int r = 0; r < 4; ++r) sums[r] = ctx->solve_state_h[r];
  return HDD_OK;
}
