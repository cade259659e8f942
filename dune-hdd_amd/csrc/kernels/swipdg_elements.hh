// dune-hdd_amd/csrc/kernels/swipdg_elements.hh -- what every SWIPDG kernel family shares: the reference
// elements and quadrature rules, coefficient / tensor access, the affine geometry, the Newton-refined fp64
// reciprocals and the 32-bit buffer-offset loaders.  (Design overview: swipdg_device.hh.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hdd.h"
#include "swipdg_kernels.hh"
#include "flattop.hh"
#include "trig_phase.hh"

namespace hdd {
namespace dev {

// ------------------------------------------------------------------------------------------------
// reference elements (Dune numbering) and shape functions
// ------------------------------------------------------------------------------------------------
struct Simplex {
  static constexpr int NV = 3, NF = 3, NB = 3;
  // vertex k of the reference simplex: (0,0), (1,0), (0,1)
  __host__ __device__ static constexpr double rv(int k, int d) { return (k == 1 + d) ? 1.0 : 0.0; }
  // faces 0:(0,1) 1:(0,2) 2:(1,2)
  __host__ __device__ static constexpr int fv(int f, int k) { return f == 0 ? k : (f == 1 ? 2 * k : 1 + k); }
  // orientation of (t_y, -t_x) w.r.t. the outer normal on the reference element
  __host__ __device__ static constexpr double face_sign(int f) { return f == 1 ? -1.0 : 1.0; }
  __device__ static inline void shape(double x, double y, double* phi, double* gx, double* gy)
  {
    phi[0] = 1.0 - x - y; phi[1] = x; phi[2] = y;
    gx[0] = -1.0; gy[0] = -1.0;
    gx[1] = 1.0;  gy[1] = 0.0;
    gx[2] = 0.0;  gy[2] = 1.0;
  }
};

struct Cube {
  static constexpr int NV = 4, NF = 4, NB = 4;
  // vertex k: (k & 1, k >> 1)
  __host__ __device__ static constexpr double rv(int k, int d) { return double((k >> d) & 1); }
  // faces 0:(0,2) 1:(1,3) 2:(0,1) 3:(2,3)
  __host__ __device__ static constexpr int fv(int f, int k)
  {
    return f == 0 ? 2 * k : (f == 1 ? 1 + 2 * k : (f == 2 ? k : 2 + k));
  }
  __host__ __device__ static constexpr double face_sign(int f) { return (f == 0 || f == 3) ? -1.0 : 1.0; }
  __device__ static inline void shape(double x, double y, double* phi, double* gx, double* gy)
  {
    phi[0] = (1 - x) * (1 - y); phi[1] = x * (1 - y); phi[2] = (1 - x) * y; phi[3] = x * y;
    gx[0] = -(1 - y); gy[0] = -(1 - x);
    gx[1] = (1 - y);  gy[1] = -x;
    gx[2] = -y;       gy[2] = (1 - x);
    gx[3] = y;        gy[3] = x;
  }
};

// The neighbour's local vertex in role r of my face f (roles name the neighbour's vertices by physical position:
// 0 / 1 = my fv(f,0) / fv(f,1), the others off the face -- see GenericPolicy), from the face's twin / reversal
// bits in face_info: the column slot of the role inside an entity/neighbour block.
template <class E>
__device__ __forceinline__ int role_slot(uint32_t finfo, int f, int r)
{
  const uint32_t inf = (finfo >> (4 * f)) & 15u;
  const int tw = int(inf & 7u);
  const bool rev = (inf & 8u) != 0u;
  const int ka = rev ? 1 : 0;
  if (r == 0) return E::fv(tw, ka);
  if (r == 1) return E::fv(tw, 1 - ka);
  if constexpr (E::NV == 3) return 3 - E::fv(tw, 0) - E::fv(tw, 1);
  else return r == 2 ? E::fv(tw ^ 1, ka) : E::fv(tw ^ 1, 1 - ka);
}

// ------------------------------------------------------------------------------------------------
// quadrature (compile-time): Gauss-Legendre on [0,1]; simplex centroid / 3-point / Dunavant-6
// ------------------------------------------------------------------------------------------------
template <int N>
struct Gauss01;
template <>
struct Gauss01<1> {
  __device__ static constexpr double s(int) { return 0.5; }
  __device__ static constexpr double w(int) { return 1.0; }
};
template <>
struct Gauss01<2> {
  __device__ static constexpr double s(int q) { return q == 0 ? 0.21132486540518711775 : 0.78867513459481288225; }
  __device__ static constexpr double w(int) { return 0.5; }
};
template <>
struct Gauss01<3> {
  __device__ static constexpr double s(int q)
  {
    return q == 0 ? 0.11270166537925831148 : (q == 1 ? 0.5 : 0.88729833462074168852);
  }
  __device__ static constexpr double w(int q) { return q == 1 ? 8.0 / 18.0 : 5.0 / 18.0; }
};

template <class E, int NQ>
struct VolRule;
template <>
struct VolRule<Simplex, 1> {
  __device__ static constexpr double x(int) { return 1.0 / 3.0; }
  __device__ static constexpr double y(int) { return 1.0 / 3.0; }
  __device__ static constexpr double w(int) { return 0.5; }
};
template <>
struct VolRule<Simplex, 3> {
  __device__ static constexpr double x(int q) { return q == 1 ? 2.0 / 3.0 : 1.0 / 6.0; }
  __device__ static constexpr double y(int q) { return q == 2 ? 2.0 / 3.0 : 1.0 / 6.0; }
  __device__ static constexpr double w(int) { return 1.0 / 6.0; }
};
template <>
struct VolRule<Simplex, 6> {  // Dunavant degree 4 (used for integrand orders 3 and 4)
  static constexpr double A = 0.44594849091596488632, WA = 0.22338158967801146570;
  static constexpr double B = 0.091576213509770743460, WB = 0.10995174365532186764;
  __device__ static constexpr double pa(int k, int d) { return k == 0 ? A : ((k == 1) == (d == 0) ? 1 - 2 * A : A); }
  __device__ static constexpr double pb(int k, int d) { return k == 0 ? B : ((k == 1) == (d == 0) ? 1 - 2 * B : B); }
  __device__ static constexpr double x(int q) { return q < 3 ? pa(q, 0) : pb(q - 3, 0); }
  __device__ static constexpr double y(int q) { return q < 3 ? pa(q, 1) : pb(q - 3, 1); }
  __device__ static constexpr double w(int q) { return q < 3 ? 0.5 * WA : 0.5 * WB; }
};
template <int NQ>
struct VolRule<Cube, NQ> {   // tensor Gauss, NQ = n*n, point q = j*n + i
  static constexpr int N = NQ == 1 ? 1 : (NQ == 4 ? 2 : 3);
  __device__ static constexpr double x(int q) { return Gauss01<N>::s(q % N); }
  __device__ static constexpr double y(int q) { return Gauss01<N>::s(q / N); }
  __device__ static constexpr double w(int q) { return Gauss01<N>::w(q % N) * Gauss01<N>::w(q / N); }
};

// ------------------------------------------------------------------------------------------------
// coefficients
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double kappa_elem(const KappaArg& k, int64_t e)
{
  return k.kind == HDD_FN_PER_ELEM ? k.per_elem[e] : k.c;
}
// |F|^-beta for beta != 1 (the 2d default is beta = 1/(d-1) = 1, taken inline as 1/|F|): out of line, so
// libm's pow and its registers stay out of the closed-form kernels' main path (P1 226 -> 191 VGPRs, Q1
// 62 -> 26 AGPR spill slots)
__device__ __attribute__((noinline)) double inv_pow(double len, double beta) { return 1.0 / pow(len, beta); }
__device__ __forceinline__ double kappa_at(const KappaArg& k, double pe, double x, double y)
{
  if (k.kind == HDD_FN_FLATTOP) return flattop_sum(k.table, k.n_table, k.c, k.b, x, y);
  return k.kind == HDD_FN_SINUSOID ? k.c + k.b * sin_phase(k.kx * x + k.ky * y) : pe;
}

typedef double dvec2 __attribute__((ext_vector_type(2)));

struct Tensor {
  double a00, a01, a11;
};
__device__ __forceinline__ Tensor tensor_of(const AssembleArgs& a, int64_t e)
{
  Tensor t;
  if (a.tkind == HDD_TENSOR_ISO_PER_ELEM) {
    const double v = a.tper[e];
    t.a00 = v; t.a01 = 0.0; t.a11 = v;
  } else if (a.tkind == HDD_TENSOR_SYM_PER_ELEM) {
    t.a00 = a.tper[e]; t.a01 = a.tper[a.n_local + e]; t.a11 = a.tper[2 * a.n_local + e];
  } else {
    t.a00 = a.tc0; t.a01 = a.tc1; t.a11 = a.tc2;
  }
  return t;
}
// (A g) . n
__device__ __forceinline__ double agn(const Tensor& A, double gx, double gy, double nx, double ny)
{
  return (A.a00 * gx + A.a01 * gy) * nx + (A.a01 * gx + A.a11 * gy) * ny;
}

// affine geometry x = v0 + J xh;  J^{-T} for the gradients
struct Geom {
  double x0, y0, j00, j01, j10, j11, det, i00, i01, i10, i11;   // i = J^{-1}
  __device__ __forceinline__ void init(double ax, double ay, double bx, double by, double cx, double cy)
  {
    x0 = ax; y0 = ay;
    j00 = bx - ax; j01 = cx - ax; j10 = by - ay; j11 = cy - ay;
    det = j00 * j11 - j01 * j10;
    const double id = 1.0 / det;
    i00 = j11 * id; i01 = -j01 * id; i10 = -j10 * id; i11 = j00 * id;
  }
  __device__ __forceinline__ void grad(double ghx, double ghy, double& gx, double& gy) const
  {
    gx = i00 * ghx + i10 * ghy;
    gy = i01 * ghx + i11 * ghy;
  }
  __device__ __forceinline__ void global(double xh, double yh, double& x, double& y) const
  {
    x = x0 + j00 * xh + j01 * yh;
    y = y0 + j10 * xh + j11 * yh;
  }
};

// ------------------------------------------------------------------------------------------------
// fp64 reciprocals / rsqrt use the hardware estimate + two Newton steps (< 1 ulp off the IEEE result);
// the oracle comparison tolerance is 1e-12 of the row maximum.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double rcp_nr(double x)
{
  double r = __builtin_amdgcn_rcp(x);
  double e = fma(-x, r, 1.0);
  r = fma(r, e, r);
  e = fma(-x, r, 1.0);
  return fma(r, e, r);
}
__device__ __forceinline__ double rsq_nr(double x)
{
  double y = __builtin_amdgcn_rsq(x);
  double h = 0.5 * x;
  y = y * fma(-h * y, y, 1.5);
  y = y * fma(-h * y, y, 1.5);
  return y;
}

// vertex (x, y) of the vertex-indexed geometry: one 16-byte load
__device__ __forceinline__ void vertex_xy(const AssembleArgs& a, int32_t v, double& x, double& y)
{
  const dvec2 p = *reinterpret_cast<const dvec2*>(a.vxy + 2 * int64_t(v));
  x = p.x;
  y = p.y;
}

template <int TK>
__device__ __forceinline__ Tensor tensor_k(const AssembleArgs& a, int64_t e)
{
  Tensor t;
  if constexpr (TK == HDD_TENSOR_ISO_PER_ELEM) {
    const double v = a.tper[e];
    t.a00 = v; t.a01 = 0.0; t.a11 = v;
  } else if constexpr (TK == HDD_TENSOR_SYM_PER_ELEM) {
    t.a00 = a.tper[e]; t.a01 = a.tper[a.n_local + e]; t.a11 = a.tper[2 * a.n_local + e];
  } else {
    t.a00 = a.tc0; t.a01 = a.tc1; t.a11 = a.tc2;
  }
  return t;
}
template <int KK>
__device__ __forceinline__ double kappa_k(const AssembleArgs& a, int64_t e)
{
  if constexpr (KK == HDD_FN_PER_ELEM) return a.kappa[0].per_elem[e];
  else return a.kappa[0].c;
}

// ------------------------------------------------------------------------------------------------
// 32-bit offset loads (vertex-indexed P1 meshes).  Each SoA array is read through a buffer resource made from its
// base pointer (wave-uniform SGPRs, hoisted out of the tile loop), the row of a [rows][n_local] array in the
// instruction's SGPR soffset and the element part in a 32-bit VGPR offset: no 64-bit VALU address arithmetic (the
// global loads cost a v_lshl_add_u64 each, the neighbours' vertex-id gathers a 64-bit multiply-add; round 5 counted
// 461 integer / select instructions beside 359 f64 ones in the C2 kernel).  The host enables vertex-indexed
// geometry only while every byte offset fits in 32 bits (n_local * 48 < 2^32, hdd_swipdg_assemble); the resources
// carry no range (num_records = 2^32 - 1).
// ------------------------------------------------------------------------------------------------
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc32(const void* p)
{
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, -1, 0x00020000);
}
__device__ __forceinline__ uint32_t ld32(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff = 0)
{
  return __builtin_amdgcn_raw_buffer_load_b32(r, int(voff), int(soff), 0);
}
__device__ __forceinline__ double ld64f(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff = 0)
{
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, int(voff), int(soff), 0));
}
__device__ __forceinline__ dvec2 ld128f(__amdgpu_buffer_rsrc_t r, uint32_t voff)
{
  return __builtin_bit_cast(dvec2, __builtin_amdgcn_raw_buffer_load_b128(r, int(voff), 0, 0));
}
// the tensor / kappa of local element e (byte offset e8 = 8 e)
template <int TK>
__device__ __forceinline__ Tensor tensor_o32(const AssembleArgs& a, uint32_t e8)
{
  Tensor t;
  if constexpr (TK == HDD_TENSOR_ISO_PER_ELEM) {
    const double v = ld64f(rsrc32(a.tper), e8);
    t.a00 = v; t.a01 = 0.0; t.a11 = v;
  } else if constexpr (TK == HDD_TENSOR_SYM_PER_ELEM) {
    const __amdgpu_buffer_rsrc_t r = rsrc32(a.tper);
    const uint32_t row = uint32_t(a.n_local) * 8u;
    t.a00 = ld64f(r, e8); t.a01 = ld64f(r, e8, row); t.a11 = ld64f(r, e8, 2u * row);
  } else {
    t.a00 = a.tc0; t.a01 = a.tc1; t.a11 = a.tc2;
  }
  return t;
}
template <int KK>
__device__ __forceinline__ double kappa_o32(const AssembleArgs& a, uint32_t e8)
{
  if constexpr (KK == HDD_FN_PER_ELEM) return ld64f(rsrc32(a.kappa[0].per_elem), e8);
  else return a.kappa[0].c;
}
__device__ __forceinline__ void vertex_xy_o32(const AssembleArgs& a, int32_t v, double& x, double& y)
{
  const dvec2 p = ld128f(rsrc32(a.vxy), uint32_t(v) * 16u);
  x = p.x;
  y = p.y;
}

typedef int ivec4 __attribute__((ext_vector_type(4)));
typedef int ivec2 __attribute__((ext_vector_type(2)));

}  // namespace dev
}  // namespace hdd
