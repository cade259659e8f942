// dune-hdd_amd/csrc/kernels/swipdg_wave_per_row.hh -- the wave-per-row fallback kernel (one workgroup per tile
// of 64 elements, wave w = local row w) for the quadrature rules no persistent policy covers, and its launch.
// Included by swipdg_assemble.hip only.
#pragma once
#include <string>
#include <type_traits>

#include "hdd_internal.hh"
#include "swipdg_elements.hh"

#ifndef HDD_MIN_WAVES_PER_EU
#define HDD_MIN_WAVES_PER_EU 4
#endif

namespace hdd {
namespace dev {

// ------------------------------------------------------------------------------------------------
// per-thread element context (loaded once, shared by all components)
// ------------------------------------------------------------------------------------------------
template <class E>
struct ElemCtx {
  double X[E::NV], Y[E::NV];
  int32_t nbr[E::NF];
  uint32_t finfo;
  Tensor A;
  Geom G;
  double adet, osgn;
  int64_t e;
  int pos_self, pos[E::NF], rowlen;
  double* img;   // LDS image of this element's row block
};

// geometry of the neighbour across face f: shared face vertices + the neighbour's non-face vertices
template <class E>
struct NbrFace {
  Geom H;
  Tensor A;
  int ta, tb, to;   // neighbour local vertices on the face (matching my fv(f,0) / fv(f,1) unless rev)
  bool rev;
};

template <class E, int F>
__device__ __forceinline__ void load_neighbor(const AssembleArgs& a, const ElemCtx<E>& c, int32_t n, NbrFace<E>& nf)
{
  const int64_t ne = a.n_local;
  constexpr int fa = E::fv(F, 0), fb = E::fv(F, 1);
  const uint32_t inf = (c.finfo >> (4 * F)) & 15u;
  const int tw = int(inf & 7u);
  nf.rev = (inf & 8u) != 0u;
  nf.ta = E::fv(tw, 0);
  nf.tb = E::fv(tw, 1);
  const double PAx = nf.rev ? c.X[fb] : c.X[fa], PAy = nf.rev ? c.Y[fb] : c.Y[fa];
  const double PBx = nf.rev ? c.X[fa] : c.X[fb], PBy = nf.rev ? c.Y[fa] : c.Y[fb];
  double NX[E::NV], NY[E::NV];
  if constexpr (E::NV == 3) {
    nf.to = 3 - nf.ta - nf.tb;
    const double Ox = a.coords[(2 * nf.to) * ne + n], Oy = a.coords[(2 * nf.to + 1) * ne + n];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      NX[k] = k == nf.ta ? PAx : (k == nf.tb ? PBx : Ox);
      NY[k] = k == nf.ta ? PAy : (k == nf.tb ? PBy : Oy);
    }
  } else {
    nf.to = -1;
    const int tc = E::fv(tw ^ 1, 0), td = E::fv(tw ^ 1, 1);
    const double Cx = a.coords[(2 * tc) * ne + n], Cy = a.coords[(2 * tc + 1) * ne + n];
    const double Dx = a.coords[(2 * td) * ne + n], Dy = a.coords[(2 * td + 1) * ne + n];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      NX[k] = k == nf.ta ? PAx : (k == nf.tb ? PBx : (k == tc ? Cx : Dx));
      NY[k] = k == nf.ta ? PAy : (k == nf.tb ? PBy : (k == tc ? Cy : Dy));
    }
  }
  nf.H.init(NX[0], NY[0], NX[1], NY[1], NX[2], NY[2]);
  nf.A = tensor_of(a, n);
}

struct FaceGeo {
  double len, nx, ny, hpow, tx, ty, xa, ya;
};

template <class E, int F>
__device__ __forceinline__ FaceGeo face_geo(const AssembleArgs& a, const ElemCtx<E>& c)
{
  constexpr int fa = E::fv(F, 0), fb = E::fv(F, 1);
  FaceGeo g;
  g.xa = c.X[fa];
  g.ya = c.Y[fa];
  g.tx = c.X[fb] - c.X[fa];
  g.ty = c.Y[fb] - c.Y[fa];
  g.len = sqrt(g.tx * g.tx + g.ty * g.ty);
  const double nsc = E::face_sign(F) * c.osgn / g.len;
  g.nx = g.ty * nsc;
  g.ny = -g.tx * nsc;
  g.hpow = a.beta == 1.0 ? g.len : pow(g.len, a.beta);
  return g;
}

// ------------------------------------------------------------------------------------------------
// row I of one component, P1 simplex with piecewise-constant coefficients: closed-form face integrals
// (exactly what the reference's order-2 Gauss rule integrates: int phi = |F|/2, int phi phi = |F|/6 (1+d_ij))
// ------------------------------------------------------------------------------------------------
template <int I>
__device__ __forceinline__ void row_simplex_pwc(const AssembleArgs& a, const ElemCtx<Simplex>& c, const KappaArg& K)
{
  using E = Simplex;
  const double ke = kappa_elem(K, c.e);
  double g[3][2];
  {
    double phi[3], ghx[3], ghy[3];
    E::shape(1.0 / 3.0, 1.0 / 3.0, phi, ghx, ghy);
#pragma unroll
    for (int k = 0; k < 3; ++k) c.G.grad(ghx[k], ghy[k], g[k][0], g[k][1]);
  }
  double self[3];
  {
    const double fac = 0.5 * c.adet;   // 1-point rule: weight 1/2 * |det J|
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double Agx = c.A.a00 * g[j][0] + c.A.a01 * g[j][1];
      const double Agy = c.A.a01 * g[j][0] + c.A.a11 * g[j][1];
      self[j] = fac * ke * (Agx * g[I][0] + Agy * g[I][1]);
    }
  }
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const int32_t n = c.nbr[f];
    if (n <= HDD_NBR_NEUMANN) continue;
    FaceGeo fg;
    double Ae[3];
    // face f as a compile-time constant for the helpers
    if (f == 0) fg = face_geo<E, 0>(a, c);
    else if (f == 1) fg = face_geo<E, 1>(a, c);
    else fg = face_geo<E, 2>(a, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) Ae[k] = agn(c.A, g[k][0], g[k][1], fg.nx, fg.ny);
    const int fa = E::fv(f, 0), fb = E::fv(f, 1), fc = 3 - fa - fb;
    const double half = 0.5 * fg.len, third = fg.len / 3.0, sixth = fg.len / 6.0;
    const double M1I = I == fc ? 0.0 : half;
    const double dm = agn(c.A, fg.nx, fg.ny, fg.nx, fg.ny);
    if (n >= 0) {
      NbrFace<E> nf;
      if (f == 0) load_neighbor<E, 0>(a, c, n, nf);
      else if (f == 1) load_neighbor<E, 1>(a, c, n, nf);
      else load_neighbor<E, 2>(a, c, n, nf);
      const double kn = kappa_elem(K, n);
      const double dp = agn(nf.A, fg.nx, fg.ny, fg.nx, fg.ny);
      const double gamma = (dp * dm) / (dp + dm);
      const double w_plus = dm / (dp + dm);
      const double w_minus = dp / (dp + dm);
      const double pen = (ke * kn * a.sigma_inner * gamma) / fg.hpow;
      double An[3];
      {
        double phi[3], ghx[3], ghy[3];
        E::shape(1.0 / 3.0, 1.0 / 3.0, phi, ghx, ghy);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double hx, hy;
          nf.H.grad(ghx[k], ghy[k], hx, hy);
          An[k] = agn(nf.A, hx, hy, fg.nx, fg.ny);
        }
      }
      // neighbour vertex matching my vertex I (only meaningful if I is on the face)
      const int mI = (I == fa) ? (nf.rev ? nf.tb : nf.ta) : (nf.rev ? nf.ta : nf.tb);
      double* out = c.img + c.pos[f] * 3;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double M1j = j == nf.to ? 0.0 : half;
        const double Mx = I == fc ? 0.0 : (j == mI ? third : (j == nf.to ? 0.0 : sixth));
        out[j] = -w_plus * kn * An[j] * M1I + w_minus * ke * Ae[I] * M1j - pen * Mx;
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double M1j = j == fc ? 0.0 : half;
        const double Mm = (I == fc || j == fc) ? 0.0 : (I == j ? third : sixth);
        self[j] += -w_minus * ke * (Ae[j] * M1I + Ae[I] * M1j) + pen * Mm;
      }
    } else {   // Dirichlet: SWIPDG::BoundaryLHS
      const double pen = (a.sigma_boundary * ke * dm) / fg.hpow;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double M1j = j == fc ? 0.0 : half;
        const double Mm = (I == fc || j == fc) ? 0.0 : (I == j ? third : sixth);
        self[j] += -ke * (Ae[j] * M1I + Ae[I] * M1j) + pen * Mm;
      }
    }
  }
  double* out = c.img + c.pos_self * 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = self[j];
}

// ------------------------------------------------------------------------------------------------
// row I of one component, generic quadrature (Q1 quads; smooth coefficients on either element)
// ------------------------------------------------------------------------------------------------
template <class E, int NQV, int NQF, int I>
__device__ __forceinline__ void row_quadrature(const AssembleArgs& a, const ElemCtx<E>& c, const KappaArg& K)
{
  constexpr int NB = E::NB, NF = E::NF;
  const double ke = kappa_elem(K, c.e);
  double self[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) self[j] = 0.0;
  // ---- LocalEvaluation::Elliptic ----
#pragma unroll
  for (int q = 0; q < NQV; ++q) {
    double phi[NB], ghx[NB], ghy[NB], gx[NB], gy[NB];
    E::shape(VolRule<E, NQV>::x(q), VolRule<E, NQV>::y(q), phi, ghx, ghy);
#pragma unroll
    for (int k = 0; k < NB; ++k) c.G.grad(ghx[k], ghy[k], gx[k], gy[k]);
    double px = 0.0, py = 0.0;
    if (smooth_kind(K.kind)) c.G.global(VolRule<E, NQV>::x(q), VolRule<E, NQV>::y(q), px, py);
    const double kap = kappa_at(K, ke, px, py);
    const double fac = VolRule<E, NQV>::w(q) * c.adet;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const double Agx = c.A.a00 * gx[j] + c.A.a01 * gy[j];
      const double Agy = c.A.a01 * gx[j] + c.A.a11 * gy[j];
      self[j] += fac * kap * (Agx * gx[I] + Agy * gy[I]);
    }
  }
  // ---- faces ----
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int32_t n = c.nbr[f];
    if (n <= HDD_NBR_NEUMANN) continue;
    FaceGeo fg;
    if (f == 0) fg = face_geo<E, 0>(a, c);
    else if (f == 1) fg = face_geo<E, 1>(a, c);
    else if (f == 2) fg = face_geo<E, 2 % NF>(a, c);
    else fg = face_geo<E, 3 % NF>(a, c);
    const int fa = E::fv(f, 0), fb = E::fv(f, 1);
    const double rax = E::rv(fa, 0), ray = E::rv(fa, 1), rbx = E::rv(fb, 0), rby = E::rv(fb, 1);
    const double dm = agn(c.A, fg.nx, fg.ny, fg.nx, fg.ny);
    if (n >= 0) {
      NbrFace<E> nf;
      if (f == 0) load_neighbor<E, 0>(a, c, n, nf);
      else if (f == 1) load_neighbor<E, 1>(a, c, n, nf);
      else if (f == 2) load_neighbor<E, 2 % NF>(a, c, n, nf);
      else load_neighbor<E, 3 % NF>(a, c, n, nf);
      const double kn = kappa_elem(K, n);
      const double dp = agn(nf.A, fg.nx, fg.ny, fg.nx, fg.ny);
      const double gamma = (dp * dm) / (dp + dm);
      const double w_plus = dm / (dp + dm);
      const double w_minus = dp / (dp + dm);
      const double sax = E::rv(nf.ta, 0), say = E::rv(nf.ta, 1), sbx = E::rv(nf.tb, 0), sby = E::rv(nf.tb, 1);
      double nbv[NB];
#pragma unroll
      for (int j = 0; j < NB; ++j) nbv[j] = 0.0;
#pragma unroll
      for (int q = 0; q < NQF; ++q) {
        const double s = Gauss01<NQF>::s(q);
        double pe[NB], ghx[NB], ghy[NB], gex[NB], gey[NB];
        E::shape(rax + s * (rbx - rax), ray + s * (rby - ray), pe, ghx, ghy);
#pragma unroll
        for (int k = 0; k < NB; ++k) c.G.grad(ghx[k], ghy[k], gex[k], gey[k]);
        const double sn = nf.rev ? 1.0 - s : s;
        double pn[NB], hhx[NB], hhy[NB], gnx[NB], gny[NB];
        E::shape(sax + sn * (sbx - sax), say + sn * (sby - say), pn, hhx, hhy);
#pragma unroll
        for (int k = 0; k < NB; ++k) nf.H.grad(hhx[k], hhy[k], gnx[k], gny[k]);
        double kme = ke, knb = kn;
        if (smooth_kind(K.kind)) {
          kme = kappa_at(K, ke, fg.xa + s * fg.tx, fg.ya + s * fg.ty);
          knb = kme;
        }
        const double pen = (kme * knb * a.sigma_inner * gamma) / fg.hpow;
        const double fac = Gauss01<NQF>::w(q) * fg.len;
        double Ae[NB], An[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          Ae[k] = agn(c.A, gex[k], gey[k], fg.nx, fg.ny);
          An[k] = agn(nf.A, gnx[k], gny[k], fg.nx, fg.ny);
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          self[j] += fac * (-w_minus * kme * Ae[j] * pe[I] - w_minus * kme * pe[j] * Ae[I] + pen * pe[j] * pe[I]);
          nbv[j] += fac * (-w_plus * knb * An[j] * pe[I] + w_minus * kme * pn[j] * Ae[I] - pen * pn[j] * pe[I]);
        }
      }
      double* out = c.img + c.pos[f] * NB;
#pragma unroll
      for (int j = 0; j < NB; ++j) out[j] = nbv[j];
    } else {   // Dirichlet
#pragma unroll
      for (int q = 0; q < NQF; ++q) {
        const double s = Gauss01<NQF>::s(q);
        double pe[NB], ghx[NB], ghy[NB], gex[NB], gey[NB];
        E::shape(rax + s * (rbx - rax), ray + s * (rby - ray), pe, ghx, ghy);
#pragma unroll
        for (int k = 0; k < NB; ++k) c.G.grad(ghx[k], ghy[k], gex[k], gey[k]);
        double kme = ke;
        if (smooth_kind(K.kind)) kme = kappa_at(K, ke, fg.xa + s * fg.tx, fg.ya + s * fg.ty);
        const double pen = (a.sigma_boundary * kme * dm) / fg.hpow;
        const double fac = Gauss01<NQF>::w(q) * fg.len;
        double Ae[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) Ae[k] = agn(c.A, gex[k], gey[k], fg.nx, fg.ny);
#pragma unroll
        for (int j = 0; j < NB; ++j) self[j] += fac * (-kme * Ae[j] * pe[I] - kme * pe[j] * Ae[I] + pen * pe[j] * pe[I]);
      }
    }
  }
  double* out = c.img + c.pos_self * NB;
#pragma unroll
  for (int j = 0; j < NB; ++j) out[j] = self[j];
}

template <class E, int NQV, int NQF, bool PWC, int I>
__device__ __forceinline__ void row(const AssembleArgs& a, const ElemCtx<E>& c, const KappaArg& K)
{
  if constexpr (PWC && std::is_same<E, Simplex>::value && NQV == 1 && NQF == 2)
    row_simplex_pwc<I>(a, c, K);
  else
    row_quadrature<E, NQV, NQF, I>(a, c, K);
}

// ------------------------------------------------------------------------------------------------
// the kernel: one workgroup = 64 consecutive owned elements x NB waves (wave w = local row w)
// ------------------------------------------------------------------------------------------------
template <class E, int NQV, int NQF, bool PWC>
__global__ void __launch_bounds__(64 * E::NB, HDD_MIN_WAVES_PER_EU)
swipdg_assemble_kernel(const AssembleArgs a)
{
  constexpr int NB = E::NB, NF = E::NF, NV = E::NV;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

  // XCD-aware tile order (bijective): hardware block b runs on XCD b % 8; each XCD gets a contiguous
  // range of tiles so the element rows above / below a tile sit in the same L2.
  const int64_t nwg = gridDim.x;
  const int64_t b = blockIdx.x;
  const int64_t q8 = nwg >> 3, r8 = nwg & 7, xcd = b & 7;
  const int64_t tile = xcd * q8 + (xcd < r8 ? xcd : r8) + (b >> 3);

  const int64_t t0 = a.own_begin + tile * 64;
  const int64_t tend = t0 + 64 < a.own_end ? t0 + 64 : a.own_end;
  const int64_t e = t0 + lane;
  const bool active = e < tend;
  const int64_t ne = a.n_local;
  const int64_t* eptr = a.elem_ptr - a.own_begin;
  const int64_t base = eptr[t0];
  const int64_t base_al = base & ~int64_t(1);          // 16-byte aligned image origin
  const int64_t tile_end = eptr[tend];

  ElemCtx<E> c;
  c.e = active ? e : t0;   // inactive tail lanes shadow a valid element; their LDS writes are skipped
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    c.X[k] = a.coords[(2 * k) * ne + c.e];
    c.Y[k] = a.coords[(2 * k + 1) * ne + c.e];
  }
#pragma unroll
  for (int f = 0; f < NF; ++f) c.nbr[f] = a.nbrs[f * ne + c.e];
  c.finfo = a.finfo[c.e];
  c.A = tensor_of(a, c.e);
  const int64_t my_off = eptr[c.e];
  c.G.init(c.X[0], c.Y[0], c.X[1], c.Y[1], c.X[2], c.Y[2]);
  c.adet = fabs(c.G.det);
  c.osgn = c.G.det > 0.0 ? 1.0 : -1.0;
  int nblk = 1;
  c.pos_self = 0;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    nblk += c.nbr[f] >= 0;
    c.pos_self += (c.nbr[f] >= 0 && c.nbr[f] < c.e);
  }
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    int p = (c.e < c.nbr[f]) ? 1 : 0;
#pragma unroll
    for (int g = 0; g < NF; ++g) p += (c.nbr[g] >= 0 && c.nbr[g] < c.nbr[f]);
    c.pos[f] = p;
  }
  c.rowlen = nblk * NB;
  // lanes past the tile end write to a scratch row after the image
  c.img = active ? lds + (my_off - base_al) + int64_t(wave) * c.rowlen
                 : lds + 64 * NB * (NF + 1) * NB + 2;

  // one component per launch (the host loops over the affine components): a component loop in here
  // would let the compiler hoist every component-invariant face quantity of all faces above the loop
  {
    const KappaArg K = a.kappa[0];
    double* out = a.vals[0];
    switch (wave) {
      case 0: row<E, NQV, NQF, PWC, 0>(a, c, K); break;
      case 1: row<E, NQV, NQF, PWC, 1>(a, c, K); break;
      case 2: row<E, NQV, NQF, PWC, 2>(a, c, K); break;
      default: if constexpr (NB > 3) row<E, NQV, NQF, PWC, NB - 1>(a, c, K); break;
    }
    __syncthreads();
    // stream the tile's contiguous row blocks [base, tile_end) out of LDS, 16 bytes per lane
    const int64_t lo = base_al, hi = tile_end;
    const int64_t n2 = (hi - lo) >> 1;
    for (int64_t k = threadIdx.x; k < n2; k += blockDim.x) {
      const int64_t gi = lo + 2 * k;
      const dvec2 v = *reinterpret_cast<const dvec2*>(lds + 2 * k);
      if (gi >= base) {
        __builtin_nontemporal_store(v, reinterpret_cast<dvec2*>(out + gi));
      } else {   // first pair straddles the tile start: only the upper value is ours
        out[gi + 1] = v.y;
      }
    }
    if (((hi - lo) & 1) && threadIdx.x == 0) out[hi - 1] = lds[hi - 1 - lo];
  }
}

// ------------------------------------------------------------------------------------------------
// host-side launch
// ------------------------------------------------------------------------------------------------
template <class E, int NQV, int NQF, bool PWC>
static hipError_t launch_t(const AssembleArgs& a, hipStream_t s)
{
  const int64_t n_own = a.own_end - a.own_begin;
  if (n_own <= 0) return hipSuccess;
  static const std::string name = [] {   // "swipdg_assemble_kernel<E, NQV, NQF, PWC>" (hdd_last_tile_kernel)
    const std::string f = __PRETTY_FUNCTION__;
    const size_t i = f.find('['), j = f.rfind(']');
    return "swipdg_assemble_kernel<" + (i == std::string::npos ? std::string("?") : f.substr(i + 1, j - i - 1)) + ">";
  }();
  hdd::last_tile_kernel_slot() = name.c_str();
  const int64_t tiles = (n_own + 63) / 64;
  // tile image (64 elements x full row blocks) + 1 alignment slot + a scratch row for tail lanes
  const size_t lds = (size_t(64) * E::NB * (E::NF + 1) * E::NB + 2 + (E::NF + 1) * E::NB) * sizeof(double);
  return per_component<false>(a, [&](const AssembleArgs& ac) {
    hipLaunchKernelGGL((swipdg_assemble_kernel<E, NQV, NQF, PWC>), dim3(unsigned(tiles)), dim3(64 * E::NB), lds, s, ac);
  });
}

}  // namespace dev
}  // namespace hdd
