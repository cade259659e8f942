// dune-hdd_amd/csrc/kernels/products.hip -- generic products of SWIPDG::init()
//
// Products of SWIPDG::init() (swipdg.hh:358-508, over_integrate = 2), one thread per matrix entry:
//   L2 phi_i phi_j, H1_SEMI grad.grad, ELLIPTIC kappa (A grad phi_j).grad phi_i, BOUNDARY_L2 on every
//   boundary face -- element-local blocks (volume pattern, row length nb);
//   PENALTY: sigma kappa^- kappa^+ gamma / |F|^beta [u][v] on inner faces and the boundary penalty on Dirichlet
//   faces -- SWIPDG face pattern (owner-computes rows: self block and one block per inner face).
// This is the family for everything the closed forms on the persistent tile driver (launch_product_fast) do not
// take: smooth kappa, hexahedra, meshes without face_info.  Written for generality, not for a roofline; the element
// helpers are those of the right-hand side (elem_affine.hh).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "elem_affine.hh"

namespace hdd {
namespace dev {

__global__ __launch_bounds__(256) void product_kernel(ProductArgs a)
{
  const int et = a.elem_type, dim = et == HDD_HEX ? 3 : 2, nb = a.nb;
  const int nf = et == HDD_SIMPLEX ? 3 : (et == HDD_CUBE ? 4 : 6);
  const bool penalty = a.kind == HDD_PRODUCT_PENALTY;
  const int64_t n_own = a.own_end - a.own_begin;
  const int64_t n = a.n_local;
  const int64_t width = penalty ? int64_t(nb) * 7 : nb;     // entries per row (upper bound for the penalty)
  const int64_t total = n_own * nb * width;
  for (int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x) {
    const int64_t k = t / (nb * width);
    const int i = int((t / width) % nb);
    const int64_t cidx = t % width;
    const int64_t e = a.own_begin + k;
    int32_t nbr[6];
    int nblk = 1;
    for (int f = 0; f < nf; ++f) {
      nbr[f] = a.nbrs[f * n + e];
      nblk += nbr[f] >= 0;
    }
    const int64_t rl = penalty ? int64_t(nb) * nblk : nb;
    if (cidx >= rl) continue;
    const int blk = int(cidx / nb), j = int(cidx % nb);
    double v0[3], J[3][3], Ji[3][3], det;
    elem_geo(a.coords, n, e, dim, v0, J, Ji, det);
    double acc = 0.0, xh[3] = {0, 0, 0}, x[3] = {0, 0, 0}, vi, vj, gi[3], gj[3];
    if (a.kind <= HDD_PRODUCT_ELLIPTIC) {
      double A[3][3];
      if (a.kind == HDD_PRODUCT_ELLIPTIC) elem_tensor(a.tkind, a.tc, a.tper, n, e, dim, A);
      const int nq = et == HDD_SIMPLEX ? a.nqv : (dim == 2 ? a.nqv * a.nqv : a.nqv * a.nqv * a.nqv);
      for (int q = 0; q < nq; ++q) {
        double w;
        if (et == HDD_SIMPLEX) {
          xh[0] = a.qv[q][0]; xh[1] = a.qv[q][1]; w = a.qv[q][3];
        } else {
          int r = q;
          w = 1.0;
          for (int c = 0; c < dim; ++c) { xh[c] = a.qv[r % a.nqv][0]; w *= a.qv[r % a.nqv][3]; r /= a.nqv; }
        }
        basis_value(et, a.degree, i, xh, vi, gi);
        basis_value(et, a.degree, j, xh, vj, gj);
        double v;
        if (a.kind == HDD_PRODUCT_L2) {
          v = vi * vj;
        } else {
          double pi[3] = {0, 0, 0}, pj[3] = {0, 0, 0};   // physical gradients J^{-T} grad_ref
          for (int c = 0; c < dim; ++c)
            for (int r = 0; r < dim; ++r) { pi[c] += Ji[r][c] * gi[r]; pj[c] += Ji[r][c] * gj[r]; }
          if (a.kind == HDD_PRODUCT_H1_SEMI) {
            v = 0.0;
            for (int c = 0; c < dim; ++c) v += pi[c] * pj[c];
          } else {
            elem_point(v0, J, dim, xh, x);
            v = 0.0;
            for (int c = 0; c < dim; ++c)
              for (int r = 0; r < dim; ++r) v += A[c][r] * pj[r] * pi[c];
            v *= fn_value(a.kappa, e, x, dim);
          }
        }
        acc += w * fabs(det) * v;
      }
      a.vals[a.elem_ptr[k] + int64_t(i) * rl + cidx] = acc;
      continue;
    }
    // face products: which element does column block `blk` belong to (blocks sorted by element id)
    int64_t col_elem = -1;
    {
      int64_t ids[7];
      int m = 0;
      ids[m++] = e;
      for (int f = 0; f < nf; ++f)
        if (nbr[f] >= 0) ids[m++] = nbr[f];
      for (int p = 1; p < m; ++p)
        for (int q = p; q > 0 && ids[q - 1] > ids[q]; --q) { const int64_t tmp = ids[q]; ids[q] = ids[q - 1]; ids[q - 1] = tmp; }
      col_elem = ids[blk];
    }
    const int nq1 = a.nq1f, nqf = dim == 2 ? nq1 : nq1 * nq1;
    double A[3][3];
    if (penalty) elem_tensor(a.tkind, a.tc, a.tper, n, e, dim, A);
    for (int f = 0; f < nf; ++f) {
      const bool inner = nbr[f] >= 0;
      if (a.kind == HDD_PRODUCT_BOUNDARY_L2 && inner) continue;
      if (penalty) {
        if (!inner && nbr[f] != HDD_NBR_DIRICHLET) continue;
        if (col_elem != e && nbr[f] != col_elem) continue;   // neighbour block: only its face
      }
      double r0[3], t1[3], t2[3], nr[3], nv[3];
      ref_face(et, f, r0, t1, t2, nr);
      const double fvol = face_normal(J, Ji, det, dim, t1, nr, nv);
      double pen_c = 1.0;   // sigma gamma / |F|^beta (without kappa)
      double v0n[3], Jn[3][3], Jin[3][3], detn;   // the neighbour's geometry (inner faces of the penalty)
      if (penalty) {
        double An[3] = {0, 0, 0}, dm = 0.0;
        for (int c = 0; c < dim; ++c)
          for (int r = 0; r < dim; ++r) An[c] += A[c][r] * nv[r];
        for (int c = 0; c < dim; ++c) dm += nv[c] * An[c];
        double gam = dm, sig = a.sigma_boundary;
        if (inner) {
          double Ao[3][3], Ano[3] = {0, 0, 0}, dp = 0.0;
          elem_tensor(a.tkind, a.tc, a.tper, n, nbr[f], dim, Ao);
          for (int c = 0; c < dim; ++c)
            for (int r = 0; r < dim; ++r) Ano[c] += Ao[c][r] * nv[r];
          for (int c = 0; c < dim; ++c) dp += nv[c] * Ano[c];
          gam = dp * dm / (dp + dm);
          sig = a.sigma_inner;
          elem_geo(a.coords, n, nbr[f], dim, v0n, Jn, Jin, detn);
        }
        pen_c = sig * gam / pow(fvol, a.beta);
      }
      for (int q = 0; q < nqf; ++q) {
        const int qs = q % nq1, qt = q / nq1;
        const double s0 = a.qf[qs][0], s1 = dim == 3 ? a.qf[qt][0] : 0.0;
        const double w = a.qf[qs][1] * (dim == 3 ? a.qf[qt][1] : 1.0);
        for (int c = 0; c < dim; ++c) xh[c] = r0[c] + s0 * t1[c] + s1 * t2[c];
        basis_value(et, a.degree, i, xh, vi, gi);
        if (!penalty) {
          basis_value(et, a.degree, j, xh, vj, gj);
          acc += w * fvol * vi * vj;
          continue;
        }
        elem_point(v0, J, dim, xh, x);
        const double ke = fn_value(a.kappa, e, x, dim);
        const double fac = w * fvol * pen_c * ke * (inner ? fn_value(a.kappa, nbr[f], x, dim) : 1.0);
        if (col_elem == e) {
          basis_value(et, a.degree, j, xh, vj, gj);
          acc += fac * vi * vj;
        } else {
          double xo[3] = {0, 0, 0};   // neighbour's reference coordinates of x
          for (int r = 0; r < dim; ++r)
            for (int c = 0; c < dim; ++c) xo[r] += Jin[r][c] * (x[c] - v0n[c]);
          basis_value(et, a.degree, j, xo, vj, gj);
          acc -= fac * vi * vj;
        }
      }
    }
    a.vals[a.elem_ptr[k] + int64_t(i) * rl + cidx] = acc;
  }
}

hipError_t launch_product(const ProductArgs& a, hipStream_t s)
{
  const int64_t width = a.kind == HDD_PRODUCT_PENALTY ? int64_t(a.nb) * 7 : a.nb;
  const int64_t total = (a.own_end - a.own_begin) * a.nb * width;
  if (total <= 0) return hipSuccess;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(product_kernel, dim3(unsigned(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hdd
