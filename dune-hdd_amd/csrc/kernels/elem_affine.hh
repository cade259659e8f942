// dune-hdd_amd/csrc/kernels/elem_affine.hh -- device helpers of one affine element, shared by the right-hand side
// (rhs.hip) and the generic products (products.hip): the data functions' values, the Lagrange basis, the geometry
// x = v0 + J xh, the symmetric tensor, the reference faces and the physical normal with the face's measure.
// Every floating-point statement stands here once, as the kernels had it inline: with -ffp-contract=on (fusion within
// an expression only) a statement rounds the same whichever kernel it is inlined into.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "swipdg_kernels.hh"
#include "flattop.hh"
#include "trig_phase.hh"

namespace hdd {
namespace dev {

// value of a data function (force, kappa, g_D, g_N) on element e at the physical point x
__device__ __forceinline__ double fn_value(const KappaArg& f, int64_t e, const double* x, int dim)
{
  switch (f.kind) {
    case HDD_FN_PER_ELEM: return f.per_elem[e];
    case HDD_FN_SINUSOID: return f.c + f.b * sin_phase(f.kx * x[0] + f.ky * x[1]);
    case HDD_FN_FLATTOP: return flattop_sum(f.table, f.n_table, f.c, f.b, x[0], x[1]);
    case HDD_FN_COS_PRODUCT:
      return f.c * cos_phase(f.kx * x[0]) * cos_phase(f.ky * x[1]) * ((dim == 3 && f.b != 0.0) ? cos_phase(f.b * x[2]) : 1.0);
    default: return f.c;
  }
}

__device__ __forceinline__ void lagr(int p, int k, double x, double& v, double& d)
{
  double val = 1.0, der = 0.0;
  for (int m = 0; m <= p; ++m) {
    if (m == k) continue;
    const double den = double(k - m) / p, f = (x - double(m) / p) / den;
    der = der * f + val / den;
    val *= f;
  }
  v = val;
  d = der;
}

// basis function i and its reference gradient at the reference point xh
__device__ inline void basis_value(int et, int p, int i, const double* xh, double& v, double* g)
{
  if (et == HDD_SIMPLEX) {
    const double l[3] = {1.0 - xh[0] - xh[1], xh[0], xh[1]};
    const double gx[3] = {-1.0, 1.0, 0.0}, gy[3] = {-1.0, 0.0, 1.0};
    v = l[i];
    g[0] = gx[i];
    g[1] = gy[i];
    return;
  }
  const int dim = et == HDD_HEX ? 3 : 2;
  const int np = p + 1;
  double lv[3], ld[3];
  int r = i;
  for (int a = 0; a < dim; ++a) {
    lagr(p, r % np, xh[a], lv[a], ld[a]);
    r /= np;
  }
  v = 1.0;
  for (int a = 0; a < dim; ++a) v *= lv[a];
  for (int b = 0; b < dim; ++b) {
    double gb = 1.0;
    for (int a = 0; a < dim; ++a) gb *= a == b ? ld[a] : lv[a];
    g[b] = gb;
  }
}

// affine geometry x = v0 + J xh of element e of the element-major coordinates [dim * nvpe][n_local] (columns of J:
// vertices 1, 2 (, 4) minus vertex 0), Ji = J^{-1}, det = det J.  (Separate arrays, not one struct: dim is a run-time
// value, and an array indexed at run time is kept in registers or LDS only as an object of its own.)
__device__ __forceinline__ void elem_geo(const double* coords, int64_t n_local, int64_t e, int dim, double* v0, double J[3][3],
                                double Ji[3][3], double& det)
{
  const int vcol[3] = {1, 2, 4};
  const int64_t n = n_local;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) J[r][c] = r == c;
  for (int c = 0; c < 3; ++c) v0[c] = 0.0;
  for (int c = 0; c < dim; ++c) v0[c] = coords[c * n + e];
  for (int j = 0; j < dim; ++j)
    for (int c = 0; c < dim; ++c) J[c][j] = coords[(dim * vcol[j] + c) * n + e] - v0[c];
  if (dim == 2) {
    det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    Ji[0][0] = J[1][1] / det; Ji[0][1] = -J[0][1] / det;
    Ji[1][0] = -J[1][0] / det; Ji[1][1] = J[0][0] / det;
  } else {
    const double c00 = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    const double c01 = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    const double c02 = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    det = J[0][0] * c00 + J[0][1] * c01 + J[0][2] * c02;
    Ji[0][0] = c00 / det; Ji[1][0] = c01 / det; Ji[2][0] = c02 / det;
    Ji[0][1] = (J[0][2] * J[2][1] - J[0][1] * J[2][2]) / det;
    Ji[1][1] = (J[0][0] * J[2][2] - J[0][2] * J[2][0]) / det;
    Ji[2][1] = (J[0][1] * J[2][0] - J[0][0] * J[2][1]) / det;
    Ji[0][2] = (J[0][1] * J[1][2] - J[0][2] * J[1][1]) / det;
    Ji[1][2] = (J[0][2] * J[1][0] - J[0][0] * J[1][2]) / det;
    Ji[2][2] = (J[0][0] * J[1][1] - J[0][1] * J[1][0]) / det;
  }
}

// physical point x of the reference point xh
__device__ __forceinline__ void elem_point(const double* v0, const double J[3][3], int dim, const double* xh, double* x)
{
  for (int c = 0; c < dim; ++c) {
    x[c] = v0[c];
    for (int j = 0; j < dim; ++j) x[c] += J[c][j] * xh[j];
  }
}

// symmetric tensor of element e: constant tc (a11 a12 a22 / a11 a12 a13 a22 a23 a33), one value per element
// (iso) or the same entries per element, tper [3 or 6][n_local]
__device__ __forceinline__ void elem_tensor(int tkind, const double* tc, const double* tper, int64_t n_local, int64_t e, int dim,
                                   double A[3][3])
{
  // (one memset, as the kernels' own `A[3][3] = {{0, ..}}` was: zeroed by nine stores from in here, rhs_kernel keeps
  // 48 more bytes per lane in scratch)
  __builtin_memset(A, 0, 9 * sizeof(double));
  if (tkind == HDD_TENSOR_ISO_PER_ELEM) {
    for (int c = 0; c < dim; ++c) A[c][c] = tper[e];
    return;
  }
  const int ns = dim == 2 ? 3 : 6;
  double cc[6];
  for (int r = 0; r < ns; ++r) cc[r] = tkind == HDD_TENSOR_SYM_PER_ELEM ? tper[r * n_local + e] : tc[r];
  if (dim == 2) {
    A[0][0] = cc[0]; A[0][1] = A[1][0] = cc[1]; A[1][1] = cc[2];
  } else {
    A[0][0] = cc[0]; A[0][1] = A[1][0] = cc[1]; A[0][2] = A[2][0] = cc[2];
    A[1][1] = cc[3]; A[1][2] = A[2][1] = cc[4]; A[2][2] = cc[5];
  }
}

// reference face f: corner r0, spanning vectors t1 (, t2), reference outer normal nr (with et and f known at compile
// time it folds to constants)
__device__ __forceinline__ void ref_face(int et, int f, double* r0, double* t1, double* t2, double* nr)
{
  for (int c = 0; c < 3; ++c) { r0[c] = 0.0; t1[c] = 0.0; t2[c] = 0.0; nr[c] = 0.0; }
  if (et == HDD_SIMPLEX) {
    // faces (v0,v1), (v0,v2), (v1,v2) of the reference triangle (0,0), (1,0), (0,1)
    const double P[3][2] = {{0, 0}, {1, 0}, {0, 1}};
    const int fv[3][2] = {{0, 1}, {0, 2}, {1, 2}};
    const double N[3][2] = {{0, -1}, {-1, 0}, {1, 1}};
    for (int c = 0; c < 2; ++c) {
      r0[c] = P[fv[f][0]][c];
      t1[c] = P[fv[f][1]][c] - P[fv[f][0]][c];
      nr[c] = N[f][c];
    }
    return;
  }
  const int dim = et == HDD_HEX ? 3 : 2;
  const int af = f >> 1, sd = f & 1;
  r0[af] = sd;
  nr[af] = sd ? 1.0 : -1.0;
  int b0 = -1, b1 = -1;
  for (int c = 0; c < dim; ++c)
    if (c != af) { if (b0 < 0) b0 = c; else b1 = c; }
  t1[b0] = 1.0;
  if (dim == 3) t2[b1] = 1.0;
}

// physical unit normal nv = J^{-T} nr / |.| of the face with reference normal nr and first spanning vector t1;
// returns the face's measure (2d: the edge's length |J t1|; 3d: Nanson, the reference face has area 1)
__device__ __forceinline__ double face_normal(const double J[3][3], const double Ji[3][3], double det, int dim,
                                              const double* t1, const double* nr, double* nv)
{
  for (int c = 0; c < 3; ++c) nv[c] = 0.0;
  for (int c = 0; c < dim; ++c)
    for (int j = 0; j < dim; ++j) nv[c] += Ji[j][c] * nr[j];
  double nn = 0.0;
  for (int c = 0; c < dim; ++c) nn += nv[c] * nv[c];
  nn = sqrt(nn);
  for (int c = 0; c < dim; ++c) nv[c] /= nn;
  if (dim == 2) {
    const double dx = J[0][0] * t1[0] + J[0][1] * t1[1], dy = J[1][0] * t1[0] + J[1][1] * t1[1];
    return sqrt(dx * dx + dy * dy);
  }
  return fabs(det) * nn;
}

}  // namespace dev
}  // namespace hdd
