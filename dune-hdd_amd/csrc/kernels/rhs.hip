// dune-hdd_amd/csrc/kernels/rhs.hip -- right-hand side of SWIPDG::init()
//
// SWIPDG right-hand side: the functionals SWIPDG::init() adds to its walk
// (dune/hdd/linearelliptic/discretizations/swipdg.hh:251-347):
//   L2Volume(f)                 b_i += int_K f phi_i
//   DirichletBoundarySWIPDG     b_i += int_F -kappa g_D (A grad phi_i).n + sigma_b kappa (n.A n) / |F|^beta g_D phi_i
//   L2Face(g_N) (Neumann faces) b_i += int_F g_N phi_i
// for P1 triangles, Q1 quadrilaterals and Q_p hexahedra.  rhs_kernel: one thread per (owned element, basis function):
// the vector has nb entries per element (work O(nb nq) per element, negligible next to the matrix), so
// the kernel is written for generality, not for a roofline; its element helpers are elem_affine.hh's, shared with the
// generic products (products.hip).  rhs2d_kernel / rhs2d_face_kernel: the P1 / Q1 hot path, one thread per element.
// Quadrature rules come from the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "elem_affine.hh"

namespace hdd {
namespace dev {

__global__ __launch_bounds__(256) void rhs_kernel(RhsArgs a)
{
  const int dim = a.elem_type == HDD_HEX ? 3 : 2;
  const int nf = a.elem_type == HDD_SIMPLEX ? 3 : (a.elem_type == HDD_CUBE ? 4 : 6);
  const int64_t n_own = a.own_end - a.own_begin;
  const int64_t total = n_own * a.nb;
  for (int64_t t = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; t < total; t += int64_t(gridDim.x) * blockDim.x) {
    const int64_t k = t / a.nb;
    const int i = int(t - k * a.nb);
    const int64_t e = a.own_begin + k;
    const int64_t n = a.n_local;
    double v0[3], J[3][3], Ji[3][3], det;
    elem_geo(a.coords, n, e, dim, v0, J, Ji, det);
    double acc = 0.0;
    double xh[3] = {0, 0, 0}, x[3] = {0, 0, 0}, v, gh[3];
    if (a.has_force) {
      for (int q = 0; q < a.nqv; ++q) {
        for (int c = 0; c < dim; ++c) xh[c] = a.qv[q][c];
        elem_point(v0, J, dim, xh, x);
        basis_value(a.elem_type, a.degree, i, xh, v, gh);
        acc += a.qv[q][3] * fabs(det) * fn_value(a.force, e, x, dim) * v;
      }
    }
    if (a.has_dirichlet || a.has_neumann) {
      for (int f = 0; f < nf; ++f) {
        const int32_t nbr = a.nbrs[f * n + e];
        const bool dir = nbr == HDD_NBR_DIRICHLET && a.has_dirichlet;
        const bool neu = nbr == HDD_NBR_NEUMANN && a.has_neumann;
        if (!dir && !neu) continue;
        double r0[3], t1[3], t2[3], nr[3], nv[3];
        ref_face(a.elem_type, f, r0, t1, t2, nr);
        const double fvol = face_normal(J, Ji, det, dim, t1, nr, nv);
        const double* qs = dir ? &a.qd[0][0] : &a.qn[0][0];
        const int nq = dir ? a.nqd : a.nqn;
        double An[3] = {0, 0, 0}, gamma = 0.0;
        if (dir) {
          double A[3][3];
          elem_tensor(a.tkind, a.tc, a.tper, n, e, dim, A);
          for (int c = 0; c < dim; ++c)
            for (int j = 0; j < dim; ++j) An[c] += A[c][j] * nv[j];
          for (int c = 0; c < dim; ++c) gamma += nv[c] * An[c];
        }
        const double hpow = dir ? pow(fvol, a.beta) : 1.0;
        for (int q = 0; q < nq; ++q) {
          const double s0 = qs[3 * q], s1 = qs[3 * q + 1], w = qs[3 * q + 2];
          for (int c = 0; c < dim; ++c) xh[c] = r0[c] + s0 * t1[c] + s1 * t2[c];
          elem_point(v0, J, dim, xh, x);
          basis_value(a.elem_type, a.degree, i, xh, v, gh);
          const double gv = w * fvol * fn_value(dir ? a.dirichlet : a.neumann, e, x, dim);
          if (dir) {
            const double kap = fn_value(a.kappa, e, x, dim);
            double gp = 0.0;   // (A grad phi_i) . n = (J^{-1} A n) . grad_ref phi_i
            for (int r = 0; r < dim; ++r) {
              double cr = 0.0;
              for (int j = 0; j < dim; ++j) cr += Ji[r][j] * An[j];
              gp += cr * gh[r];
            }
            acc += gv * (-kap * gp + a.sigma_boundary * kap * gamma / hpow * v);
          } else {
            acc += gv * v;
          }
        }
      }
    }
    a.out[t] = acc;
  }
}

// ---------------------------------------------------------------------------------------------------
// P1 / Q1 right-hand side, one thread per element: the geometry, the functions' values at the quadrature
// points and the face data are evaluated once per element (rhs_kernel above repeats them per basis
// function), the nb values of the element are accumulated in registers.  Same rules and formulas.
// ---------------------------------------------------------------------------------------------------
template <bool TRI>
__device__ __forceinline__ void rhs2d_shape(double x, double y, double* v, double* gx, double* gy)
{
  if constexpr (TRI) {
    v[0] = 1.0 - x - y; v[1] = x; v[2] = y;
    gx[0] = -1.0; gy[0] = -1.0; gx[1] = 1.0; gy[1] = 0.0; gx[2] = 0.0; gy[2] = 1.0;
  } else {
    v[0] = (1 - x) * (1 - y); v[1] = x * (1 - y); v[2] = (1 - x) * y; v[3] = x * y;
    gx[0] = -(1 - y); gy[0] = -(1 - x); gx[1] = 1 - y; gy[1] = -x; gx[2] = -y; gy[2] = 1 - x; gx[3] = y; gy[3] = x;
  }
}

// vertices 0, 1, 2 of an element (they span its affine map)
struct Verts2 {
  double x0, y0, x1, y1, x2, y2;
};

// VX: by the element's vertex ids from the 16-byte vertex rows; else element e of the element-major coordinates
template <bool VX>
__device__ __forceinline__ Verts2 rhs2d_vertices(const RhsArgs& a, int64_t e, int32_t vi0, int32_t vi1, int32_t vi2)
{
  if constexpr (VX) {
    const double2 p0 = reinterpret_cast<const double2*>(a.vxy)[vi0];
    const double2 p1 = reinterpret_cast<const double2*>(a.vxy)[vi1];
    const double2 p2 = reinterpret_cast<const double2*>(a.vxy)[vi2];
    return Verts2{p0.x, p0.y, p1.x, p1.y, p2.x, p2.y};
  } else {
    const int64_t n = a.n_local;
    return Verts2{a.coords[e], a.coords[n + e], a.coords[2 * n + e], a.coords[3 * n + e], a.coords[4 * n + e],
                  a.coords[5 * n + e]};
  }
}

// Dirichlet / Neumann faces of element e, added to acc in face order (the same rounding wherever it runs).  The
// reference face is elem_affine.hh's (constants once f is unrolled); the arithmetic is this path's own scalar 2d
// form, not the generic 3 x 3 loops: its registers decide the face kernel's occupancy.
template <bool TRI>
__device__ __forceinline__ void rhs2d_faces(const RhsArgs& a, int64_t e, double x0, double y0, double j00, double j10,
                                            double j01, double j11, double det, double* acc)
{
  constexpr int NB = TRI ? 3 : 4, NF = TRI ? 3 : 4;
  const int64_t n = a.n_local;
  double v[NB], gx[NB], gy[NB], xq[2];
  const double i00 = j11 / det, i01 = -j01 / det, i10 = -j10 / det, i11 = j00 / det;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int32_t nbr = a.nbrs[f * n + e];
    const bool dir = nbr == HDD_NBR_DIRICHLET && a.has_dirichlet;
    const bool neu = nbr == HDD_NBR_NEUMANN && a.has_neumann;
    if (!dir && !neu) continue;
    double r0[3], t1[3], t2[3], nr[3];
    ref_face(TRI ? HDD_SIMPLEX : HDD_CUBE, f, r0, t1, t2, nr);
    double nvx = i00 * nr[0] + i10 * nr[1], nvy = i01 * nr[0] + i11 * nr[1];
    const double nn = sqrt(nvx * nvx + nvy * nvy);
    nvx /= nn;
    nvy /= nn;
    const double dx = j00 * t1[0] + j01 * t1[1], dy = j10 * t1[0] + j11 * t1[1];
    const double fvol = sqrt(dx * dx + dy * dy);
    const double* qs = dir ? &a.qd[0][0] : &a.qn[0][0];
    const int nq = dir ? a.nqd : a.nqn;
    double cr0 = 0.0, cr1 = 0.0, gamma = 0.0, hpow = 1.0;
    if (dir) {
      double A00, A01, A11;
      if (a.tkind == HDD_TENSOR_ISO_PER_ELEM) {
        A00 = A11 = a.tper[e];
        A01 = 0.0;
      } else if (a.tkind == HDD_TENSOR_SYM_PER_ELEM) {
        A00 = a.tper[e]; A01 = a.tper[n + e]; A11 = a.tper[2 * n + e];
      } else {
        A00 = a.tc[0]; A01 = a.tc[1]; A11 = a.tc[2];
      }
      const double Anx = A00 * nvx + A01 * nvy, Any = A01 * nvx + A11 * nvy;
      gamma = nvx * Anx + nvy * Any;
      cr0 = i00 * Anx + i01 * Any;   // (A grad phi_i) . n = (J^{-1} A n) . grad_ref phi_i
      cr1 = i10 * Anx + i11 * Any;
      hpow = a.beta == 1.0 ? fvol : pow(fvol, a.beta);   // 2d: beta = 1/(d-1) = 1 (pow(x, 1) = x exactly)
    }
    for (int q = 0; q < nq; ++q) {
      const double s0 = qs[3 * q], w = qs[3 * q + 2];
      const double xh = r0[0] + s0 * t1[0], yh = r0[1] + s0 * t1[1];
      xq[0] = x0 + j00 * xh + j01 * yh;
      xq[1] = y0 + j10 * xh + j11 * yh;
      rhs2d_shape<TRI>(xh, yh, v, gx, gy);
      const double gv = w * fvol * fn_value(dir ? a.dirichlet : a.neumann, e, xq, 2);
      if (dir) {
        const double kap = fn_value(a.kappa, e, xq, 2);
        const double pen = a.sigma_boundary * kap * gamma / hpow;
#pragma unroll
        for (int i = 0; i < NB; ++i) acc[i] += gv * (-kap * (cr0 * gx[i] + cr1 * gy[i]) + pen * v[i]);
      } else {
#pragma unroll
        for (int i = 0; i < NB; ++i) acc[i] += gv * v[i];
      }
    }
  }
}

// Thread per element (VALU-bound: the force's cos products at the quadrature points).  VX: the vertex-indexed
// geometry (vertex ids + 16-byte vertex rows) instead of the element-major coordinates -- neutral here (same
// box 0.1345 ms both), kept so that one mesh serves every kernel.  (Staging the chunk's values in LDS for
// 16-byte stores was slower: 0.102 -> 0.135 ms.)
// NQ > 0: the force's volume rule has NQ points (unrolled: the points' trig evaluations are independent and
// interleave); FK: the force kind at compile time (-1: any, by a run-time switch)
template <bool TRI, bool VX, int NQ = 0, int FK = -1, bool SPLIT = false>
__global__ __launch_bounds__(256) void rhs2d_kernel(RhsArgs a)
{
  constexpr int NB = TRI ? 3 : 4, NF = TRI ? 3 : 4;
  const int64_t n_own = a.own_end - a.own_begin;
  const int64_t n = a.n_local;
  for (int64_t k = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; k < n_own; k += int64_t(gridDim.x) * blockDim.x) {
    const int64_t e = a.own_begin + k;
    int32_t vi0 = 0, vi1 = 0, vi2 = 0;
    if constexpr (VX) {
      vi0 = a.ev[e]; vi1 = a.ev[n + e]; vi2 = a.ev[2 * n + e];
    }
    const Verts2 p = rhs2d_vertices<VX>(a, e, vi0, vi1, vi2);
    const double x0 = p.x0, y0 = p.y0;
    const double j00 = p.x1 - x0, j10 = p.y1 - y0;   // vertex 1 - vertex 0
    const double j01 = p.x2 - x0, j11 = p.y2 - y0;   // vertex 2 - vertex 0
    const double det = j00 * j11 - j01 * j10, adet = fabs(det);
    double acc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[i] = 0.0;
    double v[NB], gx[NB], gy[NB], xq[2];
    // cos products on elements small against the wavelength (wave-uniform): one sincos per direction and
    // element, Taylor offsets per point (trig_phase.hh)
    [[maybe_unused]] double sx0 = 0.0, cx0 = 0.0, sy0 = 0.0, cy0 = 0.0;
    [[maybe_unused]] bool near = false, tiny = false;
    if constexpr (FK == HDD_FN_COS_PRODUCT && NQ > 0) {
      const double kx = a.force.kx, ky = a.force.ky;
      const double dm = fmax(fabs(kx * j00) + fabs(kx * j01), fabs(ky * j10) + fabs(ky * j11));
      near = __all(dm <= SMALL_PHASE);
      tiny = __all(dm <= TINY_PHASE) && !a.no_tiny;
      if (near) {
        sincos_phase(kx * x0, sx0, cx0);
        sincos_phase(ky * y0, sy0, cy0);
      }
    }
    auto vol_point = [&](int q) {
      const double xh = a.qv[q][0], yh = a.qv[q][1];
      xq[0] = x0 + j00 * xh + j01 * yh;
      xq[1] = y0 + j10 * xh + j11 * yh;
      rhs2d_shape<TRI>(xh, yh, v, gx, gy);
      double f;
      if constexpr (FK == HDD_FN_COS_PRODUCT) {
        if (tiny)
          f = a.force.c * cos_tiny(sx0, cx0, a.force.kx * (j00 * xh + j01 * yh)) *
              cos_tiny(sy0, cy0, a.force.ky * (j10 * xh + j11 * yh));
        else if (near)
          f = a.force.c * cos_near(sx0, cx0, a.force.kx * (j00 * xh + j01 * yh)) *
              cos_near(sy0, cy0, a.force.ky * (j10 * xh + j11 * yh));
        else
          f = a.force.c * cos_phase(a.force.kx * xq[0]) * cos_phase(a.force.ky * xq[1]);
      }
      else f = fn_value(a.force, e, xq, 2);
      const double fv = a.qv[q][3] * adet * f;
#pragma unroll
      for (int i = 0; i < NB; ++i) acc[i] += fv * v[i];
    };
    if (a.has_force) {
      if constexpr (NQ > 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) vol_point(q);
      } else {
        for (int q = 0; q < a.nqv; ++q) vol_point(q);
      }
    }
    if (a.has_dirichlet || a.has_neumann) {
      if constexpr (SPLIT) {
        // boundary elements (~0.4 % at C2) go to rhs2d_face_kernel: the face code's registers (fused, unrolled rule:
        // 205 VGPRs for P1, 256 for Q1, 2 waves per SIMD) stay out of this kernel (68-72 VGPRs and 7 waves per SIMD
        // for P1, 134-138 and 3 for Q1; every instantiation: profiles/r13/rhs/kernel_resources.txt)
        bool bnd = false;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          const int32_t nbr = a.nbrs[f * n + e];
          bnd |= (nbr == HDD_NBR_DIRICHLET && a.has_dirichlet) || (nbr == HDD_NBR_NEUMANN && a.has_neumann);
        }
        const uint64_t m = __ballot(bnd);
        if (m) {   // one atomic per wave
          const int lead = __ffsll((unsigned long long)m) - 1;
          uint32_t base = 0;
          if (int(__lane_id()) == lead) base = atomicAdd(a.bnd_list, uint32_t(__popcll(m)));
          base = __shfl(base, lead);
          const uint32_t slot = base + uint32_t(__popcll(m & ((1ull << __lane_id()) - 1)));
          // (the list holds n_own entries: a count left over from an interrupted call cannot write past it)
          if (bnd && slot < uint32_t(a.own_end - a.own_begin))   // the vertex ids ride along: the face kernel's
            reinterpret_cast<uint4*>(a.bnd_list + RHS_LIST_OFS)[slot] =   // geometry is one load from its entry
                make_uint4(uint32_t(k), uint32_t(vi0), uint32_t(vi1), uint32_t(vi2));
        }
      } else {
        rhs2d_faces<TRI>(a, e, x0, y0, j00, j10, j01, j11, det, acc);
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) __builtin_nontemporal_store(acc[i], a.out + k * NB + i);
  }
}

// the faces of the elements rhs2d_kernel<.., SPLIT> listed, added to their stored volume values in the same
// order as the fused kernel (bit-identical).  The last workgroup to finish resets the list's counters for the
// next call (no memset launch per call).
template <bool TRI, bool VX>
__global__ __launch_bounds__(256) void rhs2d_face_kernel(RhsArgs a)
{
  constexpr int NB = TRI ? 3 : 4;
  const uint4* list = reinterpret_cast<const uint4*>(a.bnd_list + RHS_LIST_OFS);
  const uint32_t n_own = uint32_t(a.own_end - a.own_begin), stride = gridDim.x * blockDim.x;
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  uint4 ent = t < n_own ? list[t] : make_uint4(0, 0, 0, 0);   // loaded beside the count (stale beyond it)
  const uint32_t count = min(__atomic_load_n(a.bnd_list, __ATOMIC_RELAXED), n_own);
  for (; t < count; t += stride) {
    const int64_t k = ent.x;
    const int64_t e = a.own_begin + k;
    const Verts2 p = rhs2d_vertices<VX>(a, e, int32_t(ent.y), int32_t(ent.z), int32_t(ent.w));
    const double j00 = p.x1 - p.x0, j10 = p.y1 - p.y0, j01 = p.x2 - p.x0, j11 = p.y2 - p.y0;
    const double det = j00 * j11 - j01 * j10;
    double acc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) acc[i] = a.out[k * NB + i];
    rhs2d_faces<TRI>(a, e, p.x0, p.y0, j00, j10, j01, j11, det, acc);
#pragma unroll
    for (int i = 0; i < NB; ++i) a.out[k * NB + i] = acc[i];
    if (t + stride < count) ent = list[t + stride];
  }
  __syncthreads();
  // no fence: a workgroup's count load has returned before its loop ended (the loop bound depends on it), and
  // the reset is seen by the next call's kernels through the kernel boundary
  if (threadIdx.x == 0) {
    if (atomicAdd(a.bnd_list + 1, 1u) == gridDim.x - 1) {   // every workgroup has read the count
      __atomic_store_n(a.bnd_list, 0u, __ATOMIC_RELAXED);
      __atomic_store_n(a.bnd_list + 1, 0u, __ATOMIC_RELAXED);
    }
  }
}

// f(bool_constant, ..) for run-time bools: one call site instantiates a kernel for every combination
template <class F>
static void with_bools(F&& f)
{
  f();
}
template <class F, class... Bools>
static void with_bools(F&& f, bool b, Bools... rest)
{
  if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

hipError_t launch_rhs(const RhsArgs& a, hipStream_t s)
{
  const int64_t n_own = a.own_end - a.own_begin;
  if (a.elem_type != HDD_HEX && n_own > 0) {
    const bool tri = a.elem_type == HDD_SIMPLEX, vx = a.ev != nullptr;
    // the ESV2007-type force (cos products) on the rules of order 4 (Dunavant 6 / Gauss 3 x 3): unrolled
    const bool unrolled = a.has_force && a.force.kind == HDD_FN_COS_PRODUCT && a.nqv == (tri ? 6 : 9) && !a.generic;
    // split: volume kernel + boundary-element list + face kernel (needs the context's list, see RhsArgs)
    const bool split = a.bnd_list && (a.has_dirichlet || a.has_neumann);
    const dim3 g(unsigned(std::min<int64_t>((n_own + 255) / 256, int64_t(a.n_cu) * 8))), b(256);
    with_bools([&](auto tri_c, auto vx_c, auto unrolled_c, auto split_c) {
      constexpr bool TRI = decltype(tri_c)::value, UNROLLED = decltype(unrolled_c)::value;
      constexpr int NQ = UNROLLED ? (TRI ? 6 : 9) : 0, FK = UNROLLED ? int(HDD_FN_COS_PRODUCT) : -1;
      hipLaunchKernelGGL((rhs2d_kernel<TRI, decltype(vx_c)::value, NQ, FK, decltype(split_c)::value>), g, b, 0, s, a);
    }, tri, vx, unrolled, split);
    hipError_t e = hipGetLastError();
    if (!split || e != hipSuccess) return e;
    // a quarter of the CUs (16 K threads: one list entry per thread at C2's 7,680 boundary elements); every
    // workgroup, busy or not, pays the finish atomic
    const dim3 gf(unsigned(std::max(1, a.n_cu / 4)));
    if (a.skip_face) {
      e = hipErrorLaunchFailure;   // error injection (tests): the face launch did not happen
    } else {
      with_bools([&](auto tri_c, auto vx_c) {
        hipLaunchKernelGGL((rhs2d_face_kernel<decltype(tri_c)::value, decltype(vx_c)::value>), gf, b, 0, s, a);
      }, tri, vx);
      e = hipGetLastError();
    }
    // the volume kernel has filled the list but no face kernel will reset it: re-arm the counters here, so the
    // next call starts from an empty list (stream-ordered behind the volume kernel)
    if (e != hipSuccess) (void)hipMemsetAsync(a.bnd_list, 0, 2 * sizeof(uint32_t), s);
    return e;
  }
  const int64_t total = n_own * a.nb;
  if (total <= 0) return hipSuccess;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(rhs_kernel, dim3(unsigned(blocks < (1 << 20) ? blocks : (1 << 20))), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dev
}  // namespace hdd
