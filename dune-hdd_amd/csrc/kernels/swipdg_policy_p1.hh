// dune-hdd_amd/csrc/kernels/swipdg_policy_p1.hh -- the P1 (triangle) policies of the persistent tile driver:
// closed-form piecewise-constant stiffness / penalty (P1PwcPolicy, the C2 kernel), smooth-kappa moments
// (P1SmoothPolicy) and its fused multi-component form (P1SmoothFusedPolicy, C3).
#pragma once
#include "swipdg_elements.hh"
#include "swipdg_policy.hh"

namespace hdd {
namespace dev {

// ------------------------------------------------------------------------------------------------
// P1 simplex, piecewise-constant coefficients: one thread per element computes all 3 rows.
//
// Face terms in "role" form: for face f with my vertices a = fv(f,0), b = fv(f,1), the neighbour's
// vertices are named by their physical position (role A = position of my a, B = position of my b,
// O = the neighbour's opposite vertex).  Then every coefficient of the entity/entity and
// entity/neighbour blocks is orientation-free, and the twin face / reversal only decides the three LDS
// column slots j(A), j(B), j(O) the entity/neighbour values are stored to.  The neighbour gradients come
// from the triangle (A, B, O) (barycentric gradients), so a face gathers only O (2 doubles), the
// neighbour tensor and, if per element, its diffusion factor.
//
// fp64 reciprocals / rsqrt: rcp_nr / rsq_nr (swipdg_elements.hh).
// ------------------------------------------------------------------------------------------------
struct P1Own {
  double X[3], Y[3];
  int32_t nbr[3];
  uint32_t finfo;
  Tensor A;
  double ke;
  int32_t vid[3];   // vertex-indexed geometry (VX): local vertex ids; X / Y then arrive with the gathers
};
struct P1Gat {
  double Ox[3], Oy[3];
  Tensor Ap[3];
  double kn[3];
  int32_t ov[3];    // VX: the neighbour's off-face vertex id; Ox / Oy arrive in the second gather stage
};

// Own-data loads of a tile (coalesced SoA).  VX: vertex ids instead of coordinates -- the vertex
// coordinates are then gathered with the neighbour data (p1_load_gat), the neighbour's off-face vertex in a
// second stage (p1_load_gat2) that the persistent driver issues after the tile's stores.  VX reads go through the
// 32-bit offset loads (swipdg_elements.hh).
template <int TK, int KK, bool VX = false>
__device__ __forceinline__ void p1_load_own(const AssembleArgs& a, int64_t e, P1Own& o)
{
  const int64_t ne = a.n_local;
  if constexpr (VX) {
    const uint32_t e4 = uint32_t(e) * 4u, row = uint32_t(ne) * 4u;
    const __amdgpu_buffer_rsrc_t rv = rsrc32(a.ev), rn = rsrc32(a.nbrs);
#pragma unroll
    for (int k = 0; k < 3; ++k) o.vid[k] = int32_t(ld32(rv, e4, uint32_t(k) * row));
#pragma unroll
    for (int f = 0; f < 3; ++f) o.nbr[f] = int32_t(ld32(rn, e4, uint32_t(f) * row));
    o.finfo = ld32(rsrc32(a.finfo), e4);
    o.A = tensor_o32<TK>(a, 2u * e4);
    o.ke = kappa_o32<KK>(a, 2u * e4);
    return;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o.X[k] = a.coords[(2 * k) * ne + e];
    o.Y[k] = a.coords[(2 * k + 1) * ne + e];
  }
#pragma unroll
  for (int f = 0; f < 3; ++f) o.nbr[f] = a.nbrs[f * ne + e];
  o.finfo = a.finfo[e];
  o.A = tensor_k<TK>(a, e);
  o.ke = kappa_k<KK>(a, e);
}

template <int TK, int KK, bool VX = false>
__device__ __forceinline__ void p1_load_gat(const AssembleArgs& a, int64_t e, P1Own& o, P1Gat& g)
{
  const int64_t ne = a.n_local;
  if constexpr (VX) {
#pragma unroll
    for (int k = 0; k < 3; ++k) vertex_xy_o32(a, o.vid[k], o.X[k], o.Y[k]);
    const uint32_t row = uint32_t(ne) * 4u;
    const __amdgpu_buffer_rsrc_t rv = rsrc32(a.ev);
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const uint32_t n = o.nbr[f] >= 0 ? uint32_t(o.nbr[f]) : uint32_t(e);   // boundary faces: harmless own reload
      // the neighbour's vertex opposite its twin face tw (Simplex faces (0,1), (0,2), (1,2)): 2 - tw (clamped, so
      // whatever a boundary face's info bits hold the offset stays inside the array)
      const uint32_t to = min(2u - ((o.finfo >> (4 * f)) & 7u), 2u);
      g.ov[f] = int32_t(ld32(rv, to * row + 4u * n));
      g.Ap[f] = tensor_o32<TK>(a, 8u * n);
      g.kn[f] = kappa_o32<KK>(a, 8u * n);
    }
    return;
  }
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const int64_t n = o.nbr[f] >= 0 ? int64_t(o.nbr[f]) : e;   // boundary faces: harmless own reload
    const uint32_t inf = (o.finfo >> (4 * f)) & 15u;
    const int tw = int(inf & 7u);
    const int to = 3 - Simplex::fv(tw, 0) - Simplex::fv(tw, 1);
    g.Ox[f] = a.coords[(2 * to) * ne + n];
    g.Oy[f] = a.coords[(2 * to + 1) * ne + n];
    g.Ap[f] = tensor_k<TK>(a, n);
    g.kn[f] = kappa_k<KK>(a, n);
  }
}
template <bool VX>
__device__ __forceinline__ void p1_load_gat2(const AssembleArgs& a, P1Gat& g)
{
  if constexpr (VX) {
#pragma unroll
    for (int f = 0; f < 3; ++f) vertex_xy_o32(a, g.ov[f], g.Ox[f], g.Oy[f]);
  }
}

// P1 closed-form per-element math on preloaded data (role form, see above); writes the row block into `img`.
// PEN: only the interior-penalty terms (the SWIPDG penalty product, swipdg.hh:462-508), no volume and no
// consistency / symmetry terms.
// the element's own block from one face: S_ij += -c (Ae_j [i != fc] + Ae_i [j != fc]) + (pen / 3 or pen / 6 on the
// face's vertex pairs), c = |F| / 2 times the consistency weight (fc: the vertex opposite the face)
__device__ __forceinline__ void p1_face_self(double (&S)[3][3], const double (&Ae)[3], int fc, double c, double penT,
                                             double penS)
{
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {   // the block is symmetric: the upper triangle (p1_compute mirrors it)
      if (i == fc && j == fc) continue;
      const double v = i == fc ? Ae[i] : (j == fc ? Ae[j] : Ae[i] + Ae[j]);
      S[i][j] = fma(-c, v, S[i][j] + (i == fc || j == fc ? 0.0 : (i == j ? penT : penS)));
    }
}

// ALLIN: the caller guarantees three interior faces (every element of a full interior tile, see the persistent
// driver): no per-face branches, the row length and block count compile-time constants
template <bool PEN = false, bool ALLIN = false>
__device__ __forceinline__ void p1_compute(const AssembleArgs& a, int64_t e, const P1Own& o, const P1Gat& gt,
                                           double* img)
{
  using E = Simplex;
  const double j00 = o.X[1] - o.X[0], j01 = o.X[2] - o.X[0], j10 = o.Y[1] - o.Y[0], j11 = o.Y[2] - o.Y[0];
  const double det = j00 * j11 - j01 * j10;
  const double id = rcp_nr(det);
  const double i00 = j11 * id, i01 = -j01 * id, i10 = -j10 * id, i11 = j00 * id;
  double g[3][2];
  g[1][0] = i00; g[1][1] = i01;
  g[2][0] = i10; g[2][1] = i11;
  g[0][0] = -i00 - i10; g[0][1] = -i01 - i11;
  double Ag[3][2];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Ag[k][0] = o.A.a00 * g[k][0] + o.A.a01 * g[k][1];
    Ag[k][1] = o.A.a01 * g[k][0] + o.A.a11 * g[k][1];
  }
  const double adet = fabs(det);
  const double osgn = det > 0.0 ? 1.0 : -1.0;
  const int32_t ei = int32_t(e);   // local ids are int32 (hdd_mesh neighbors): 32-bit compares
  int nblk = 1, pos_self = 0, pos[3];
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    nblk += ALLIN || o.nbr[f] >= 0;
    pos_self += ((ALLIN || o.nbr[f] >= 0) && o.nbr[f] < ei);
  }
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    int p = (ei < o.nbr[f]) ? 1 : 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) p += ((ALLIN || o.nbr[q] >= 0) && o.nbr[q] < o.nbr[f]);
    pos[f] = p;
  }
  const int rowlen = ALLIN ? 12 : nblk * 3;
  const double ke = o.ke;
  double S[3][3];
  {
    const double fac = PEN ? 0.0 : 0.5 * adet * ke;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i; j < 3; ++j) S[i][j] = fac * (Ag[j][0] * g[i][0] + Ag[j][1] * g[i][1]);   // symmetric A
  }
  constexpr double CS = PEN ? 0.0 : 1.0;   // consistency / symmetry terms on (stiffness) or off (penalty)
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const int32_t n = o.nbr[f];
    if (!ALLIN && n <= HDD_NBR_NEUMANN) continue;
    const int fa = E::fv(f, 0), fb = E::fv(f, 1), fc = 3 - fa - fb;
    const double tx = o.X[fb] - o.X[fa], ty = o.Y[fb] - o.Y[fa];
    const double il = rsq_nr(tx * tx + ty * ty);
    const double len = (tx * tx + ty * ty) * il;
    const double nsc = E::face_sign(f) * osgn * il;
    const double nx = ty * nsc, ny = -tx * nsc;
    double Ae[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) Ae[k] = Ag[k][0] * nx + Ag[k][1] * ny;
    const double dm = agn(o.A, nx, ny, nx, ny);
    const double ihp = a.beta == 1.0 ? il : inv_pow(len, a.beta);
    const double half = 0.5 * len, third = len * (1.0 / 3.0), sixth = len * (1.0 / 6.0);
    if (ALLIN || n >= 0) {
      const uint32_t inf = (o.finfo >> (4 * f)) & 15u;
      const int tw = int(inf & 7u);
      const bool rev = (inf & 8u) != 0u;
      const int ta = E::fv(tw, 0), tb = E::fv(tw, 1), to = 3 - ta - tb;
      const double Ox = gt.Ox[f], Oy = gt.Oy[f];
      const Tensor Ap = gt.Ap[f];
      const double kn = gt.kn[f];
      const double dp = agn(Ap, nx, ny, nx, ny);
      const double rs = rcp_nr(dp + dm);
      const double gamma = (dp * dm) * rs;
      const double w_plus = dm * rs, w_minus = dp * rs;
      const double pen = (ke * kn * a.sigma_inner * gamma) * ihp;
      const double Ax = o.X[fa], Ay = o.Y[fa], Bx = o.X[fb], By = o.Y[fb];
      const double iD = rcp_nr((Bx - Ax) * (Oy - Ay) - (By - Ay) * (Ox - Ax));
      const double mx = Ap.a00 * nx + Ap.a01 * ny, my = Ap.a01 * nx + Ap.a11 * ny;
      const double AnA = ((By - Oy) * mx + (Ox - Bx) * my) * iD;
      const double AnB = ((Oy - Ay) * mx + (Ax - Ox) * my) * iD;
      const double AnO = ((Ay - By) * mx + (Bx - Ax) * my) * iD;
      const int jA = rev ? tb : ta, jB = rev ? ta : tb;
      // the face's constants folded once (half = |F| / 2, third, sixth = the P1 trace mass entries), so every entry
      // is a two-FMA chain (fc, fa, fb are compile-time per unrolled face)
      const double cplh = -w_plus * kn * CS * half;
      const double symh = w_minus * ke * CS * half;
      const double penT = pen * third, penS = pen * sixth;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        double* row = img + i * rowlen + pos[f] * 3;
        if (i == fc) {
          row[jA] = symh * Ae[i];
          row[jB] = symh * Ae[i];
          row[to] = 0.0;
        } else {
          row[jA] = fma(cplh, AnA, fma(symh, Ae[i], -(i == fa ? penT : penS)));
          row[jB] = fma(cplh, AnB, fma(symh, Ae[i], -(i == fb ? penT : penS)));
          row[to] = cplh * AnO;
        }
      }
      p1_face_self(S, Ae, fc, symh, penT, penS);
    } else {
      const double pen = (a.sigma_boundary * ke * dm) * ihp;
      p1_face_self(S, Ae, fc, ke * CS * half, pen * third, pen * sixth);
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) img[i * rowlen + pos_self * 3 + j] = j >= i ? S[i][j] : S[j][i];
}

// P1 simplex, piecewise-constant coefficients: the closed-form policy (p1_compute above)
template <int TK, int KK, bool PEN = false, bool VX = false>
struct P1PwcPolicy : PolicyDefaults {
  static constexpr int NB = 3, NF = 3;
  static constexpr int RB = 36;
  // store-bound.  Element-major geometry: 8 tiles per CU since the out-of-line pow (191 VGPRs, 2 waves per
  // SIMD): C2 0.310 / 0.305 vs 0.312 / 0.314 ms at 4 (profiles/r01/s3/sweep_wgcu_s3.log).  Vertex-indexed
  // geometry: 4 (one wave per SIMD): C2 0.230-0.237 ms vs 0.246-0.247 at 8, 0.242 at 6, 0.256 at 3
  // (same box, profiles/r02/s2/ab_wgcu_vx*)
  static constexpr int WGCU = VX ? 4 : 8, MINW = 1;
  static constexpr bool PAD = false;          // store-bound: its 4-way write conflicts stay hidden
  using Own = P1Own;
  using Gat = P1Gat;
  __device__ static void load_own(const AssembleArgs& a, int64_t e, Own& o) { p1_load_own<TK, KK, VX>(a, e, o); }
  __device__ static void load_gat(const AssembleArgs& a, int64_t e, Own& o, Gat& g) { p1_load_gat<TK, KK, VX>(a, e, o, g); }
  __device__ static void load_gat2(const AssembleArgs& a, Gat& g) { p1_load_gat2<VX>(a, g); }
  __device__ static int n_interior(const Own& o) { return int(o.nbr[0] >= 0) + int(o.nbr[1] >= 0) + int(o.nbr[2] >= 0); }
  __device__ static void compute(const AssembleArgs& a, int64_t e, const Own& o, const Gat& g, double* img)
  {
    p1_compute<PEN>(a, e, o, g, img);
  }
  // full interior tiles (64 elements, three interior faces each: tile length 64 RB): branch-free faces, the image
  // layout static (lane l's row block at l RB)
  static constexpr bool FULLTILE = true;
  __device__ static void compute_full(const AssembleArgs& a, int64_t e, const Own& o, const Gat& g, double* img)
  {
    p1_compute<PEN, true>(a, e, o, g, img);
  }
};

// ------------------------------------------------------------------------------------------------
// P1 with a smooth diffusion factor (OS2014 sinusoid, C3): kappa moments.
//
// P1 gradients, and hence (A grad phi) . n, are constant on an element, so every integrand is kappa (or
// kappa^2 in the interior penalty, kappa^- kappa^+ with one smooth kappa) times a polynomial of the trace:
//   volume   int kappa grad phi_j . A grad phi_i  = |det J| (sum_q w_q kappa(x_q)) g_i . A g_j      (Dunavant 6)
//   face     int kappa phi_i        = |F| sum_q w_q kappa(x_q) phi_i(s_q)                         (Gauss 3)
//            int kappa^m phi_i phi_j = |F| sum_q w_q kappa(x_q)^m phi_i(s_q) phi_j(s_q)  (m = 2 inner, 1 Dirichlet)
// The moments use the reference's points and weights (the same rules as GenericPolicy: integrand orders
// ord kappa + 0 / ord kappa + 2 with ord kappa = 3), so the entries equal the quadrature form up to
// rounding, at 15 kappa evaluations and the P1 closed-form entry count per element.
// ------------------------------------------------------------------------------------------------
template <int TK, bool VX = false, int KK = HDD_FN_SINUSOID>   // KK: the smooth kind (SINUSOID, FLATTOP)
struct P1SmoothPolicy : PolicyDefaults {
  static constexpr int NB = 3, NF = 3;
  static constexpr int RB = 36;
  // 8 tiles per CU at <= 256 registers: 0.201 ms per C3 component vs 0.231 at 4 (and 0.230 for the
  // quadrature policy at 8; profiles/r01/s2/ab_p1s.log)
  static constexpr int WGCU = 8, MINW = 2;
  static constexpr bool PAD = false;
  using Own = P1Own;
  using Gat = P1Gat;
  __device__ static void load_own(const AssembleArgs& a, int64_t e, Own& o) { p1_load_own<TK, HDD_FN_CONST, VX>(a, e, o); }
  __device__ static void load_gat(const AssembleArgs& a, int64_t e, Own& o, Gat& g)
  {
    p1_load_gat<TK, HDD_FN_CONST, VX>(a, e, o, g);
  }
  __device__ static void load_gat2(const AssembleArgs& a, Gat& g) { p1_load_gat2<VX>(a, g); }
  __device__ static int n_interior(const Own& o) { return int(o.nbr[0] >= 0) + int(o.nbr[1] >= 0) + int(o.nbr[2] >= 0); }

  __device__ static void compute(const AssembleArgs& a, int64_t e, const Own& o, const Gat& gt, double* img)
  {
    const KappaArg& K = a.kappa[0];
    auto kap = [&](double x, double y) {
      if constexpr (KK == HDD_FN_FLATTOP) return flattop_sum(K.table, K.n_table, K.c, K.b, x, y);
      return K.c + K.b * sin_phase(K.kx * x + K.ky * y);
    };
    const double j00 = o.X[1] - o.X[0], j01 = o.X[2] - o.X[0], j10 = o.Y[1] - o.Y[0], j11 = o.Y[2] - o.Y[0];
    double kv = 0.0;   // sum_q w_q kappa(x_q), Dunavant 6
    if constexpr (KK == HDD_FN_SINUSOID) {   // small elements: one reduction per element (see the fused policy)
      const double d1 = K.kx * j00 + K.ky * j10, d2 = K.kx * j01 + K.ky * j11;
      if (__all(fabs(d1) + fabs(d2) <= SMALL_PHASE)) {
        double s0, c0;
        sincos_phase(K.kx * o.X[0] + K.ky * o.Y[0], s0, c0);
#pragma unroll
        for (int q = 0; q < 6; ++q)
          kv += VolRule<Simplex, 6>::w(q) *
                (K.c + K.b * sin_near(s0, c0, VolRule<Simplex, 6>::x(q) * d1 + VolRule<Simplex, 6>::y(q) * d2));
        const double dv[3] = {0.0, d1, d2};
        emit(a, e, o, gt, img, kv, [&](int f, double, double, int q) {
          const double da = dv[Simplex::fv(f, 0)], db = dv[Simplex::fv(f, 1)];
          return K.c + K.b * sin_near(s0, c0, da + Gauss01<3>::s(q) * (db - da));
        });
        return;
      }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const double xh = VolRule<Simplex, 6>::x(q), yh = VolRule<Simplex, 6>::y(q);
      kv += VolRule<Simplex, 6>::w(q) * kap(o.X[0] + j00 * xh + j01 * yh, o.Y[0] + j10 * xh + j11 * yh);
    }
    emit(a, e, o, gt, img, kv, [&](int f, double x, double y, int) { return kap(x, y); });
  }

  // the entries from the volume moment kv = sum_q w_q kappa(x_q) and kappa at the face Gauss points,
  // KF(f, x, y, q) (point q of face f at (x, y), from vertex a to b); ALLIN: three interior faces (full tiles of the
  // persistent driver, as p1_compute)
  template <bool ALLIN = false, class KFace>
  __device__ static void emit(const AssembleArgs& a, int64_t e, const Own& o, const Gat& gt, double* img, double kv,
                              KFace KF)
  {
    double* imgs[1] = {img};
    const double kvs[1] = {kv};
    emitN<1, ALLIN>(a, e, o, gt, imgs, kvs, [&](int, int f, double x, double y, int q) { return KF(f, x, y, q); });
  }

  // NC components at once (the fused C3 policy): the geometry -- Jacobian, gradients, face normals and lengths, the
  // neighbour's gradients, the harmonic weights -- is evaluated once and each component's entries (its own kappa
  // moments) written into its image img[c]; per component the arithmetic is exactly that of emit (NC = 1).
  // KF(c, f, x, y, q): component c's kappa at point q of face f.
  template <int NC, bool ALLIN = false, class KFace>
  __device__ static void emitN(const AssembleArgs& a, int64_t e, const Own& o, const Gat& gt, double* const (&img)[NC],
                               const double (&kv)[NC], KFace KF)
  {
    using E = Simplex;
    const double j00 = o.X[1] - o.X[0], j01 = o.X[2] - o.X[0], j10 = o.Y[1] - o.Y[0], j11 = o.Y[2] - o.Y[0];
    const double det = j00 * j11 - j01 * j10;
    const double id = rcp_nr(det);
    const double i00 = j11 * id, i01 = -j01 * id, i10 = -j10 * id, i11 = j00 * id;
    double g[3][2];
    g[1][0] = i00; g[1][1] = i01;
    g[2][0] = i10; g[2][1] = i11;
    g[0][0] = -i00 - i10; g[0][1] = -i01 - i11;
    double Ag[3][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Ag[k][0] = o.A.a00 * g[k][0] + o.A.a01 * g[k][1];
      Ag[k][1] = o.A.a01 * g[k][0] + o.A.a11 * g[k][1];
    }
    const double adet = fabs(det);
    const double osgn = det > 0.0 ? 1.0 : -1.0;
    const int32_t ei = int32_t(e);   // 32-bit compares (local ids are int32)
    int nblk = 1, pos_self = 0, pos[3];
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      nblk += ALLIN || o.nbr[f] >= 0;
      pos_self += ((ALLIN || o.nbr[f] >= 0) && o.nbr[f] < ei);
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      int p = (ei < o.nbr[f]) ? 1 : 0;
#pragma unroll
      for (int q = 0; q < 3; ++q) p += ((ALLIN || o.nbr[q] >= 0) && o.nbr[q] < o.nbr[f]);
      pos[f] = p;
    }
    const int rowlen = ALLIN ? 12 : nblk * 3;
    // the own block is symmetric (volume g_i.A g_j, face terms symmetric in i, j): its upper triangle, mirrored at
    // the end
    double S[NC][3][3];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double vol = adet * kv[c];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) S[c][i][j] = vol * (Ag[j][0] * g[i][0] + Ag[j][1] * g[i][1]);
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const int32_t n = o.nbr[f];
      if (!ALLIN && n <= HDD_NBR_NEUMANN) continue;
      const int fa = E::fv(f, 0), fb = E::fv(f, 1), fc = 3 - fa - fb;
      const double Ax = o.X[fa], Ay = o.Y[fa], Bx = o.X[fb], By = o.Y[fb];
      const double tx = Bx - Ax, ty = By - Ay;
      const double il = rsq_nr(tx * tx + ty * ty);
      const double len = (tx * tx + ty * ty) * il;
      const double nsc = E::face_sign(f) * osgn * il;
      const double nx = ty * nsc, ny = -tx * nsc;
      double Ae[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) Ae[k] = Ag[k][0] * nx + Ag[k][1] * ny;
      const double dm = agn(o.A, nx, ny, nx, ny);
      const double ihp = a.beta == 1.0 ? il : inv_pow(len, a.beta);
      const bool inner = ALLIN || n >= 0;
      // moments over the face's Gauss 3 points (s from vertex a to vertex b), per component
      double k1a[NC], k1b[NC], qaa[NC], qab[NC], qbb[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        k1a[c] = k1b[c] = qaa[c] = qab[c] = qbb[c] = 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const double sq = Gauss01<3>::s(q), wq = Gauss01<3>::w(q) * len;
          const double k = KF(c, f, Ax + sq * tx, Ay + sq * ty, q);
          const double kk = inner ? k * k : k;
          k1a[c] += wq * k * (1.0 - sq);
          k1b[c] += wq * k * sq;
          qaa[c] += wq * kk * (1.0 - sq) * (1.0 - sq);
          qab[c] += wq * kk * sq * (1.0 - sq);
          qbb[c] += wq * kk * sq * sq;
        }
      }
      auto M1 = [&](int c, int i) { return i == fa ? k1a[c] : (i == fb ? k1b[c] : 0.0); };
      auto MM = [&](int c, int i, int j) {
        return (i == fc || j == fc) ? 0.0 : (i != j ? qab[c] : (i == fa ? qaa[c] : qbb[c]));
      };
      if (inner) {
        const uint32_t inf = (o.finfo >> (4 * f)) & 15u;
        const int tw = int(inf & 7u);
        const bool rev = (inf & 8u) != 0u;
        const int ta = E::fv(tw, 0), tb = E::fv(tw, 1), to = 3 - ta - tb;
        const double Ox = gt.Ox[f], Oy = gt.Oy[f];
        const Tensor Ap = gt.Ap[f];
        const double dp = agn(Ap, nx, ny, nx, ny);
        const double rs = rcp_nr(dp + dm);
        const double gamma = (dp * dm) * rs;
        const double w_plus = dm * rs, w_minus = dp * rs;
        const double pc = (a.sigma_inner * gamma) * ihp;
        const double iD = rcp_nr((Bx - Ax) * (Oy - Ay) - (By - Ay) * (Ox - Ax));
        const double mx = Ap.a00 * nx + Ap.a01 * ny, my = Ap.a01 * nx + Ap.a11 * ny;
        const double AnA = ((By - Oy) * mx + (Ox - Bx) * my) * iD;
        const double AnB = ((Oy - Ay) * mx + (Ax - Ox) * my) * iD;
        const double AnO = ((Ay - By) * mx + (Bx - Ax) * my) * iD;
        const int jA = rev ? tb : ta, jB = rev ? ta : tb;
        // per-face products once: each entry a two-FMA chain
        const double wA = -w_plus * AnA, wB = -w_plus * AnB, wO = -w_plus * AnO;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const double wka = w_minus * k1a[c], wkb = w_minus * k1b[c];
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            double* row = img[c] + i * rowlen + pos[f] * 3;
            const double m1i = M1(c, i);
            row[jA] = fma(wA, m1i, fma(Ae[i], wka, -pc * MM(c, i, fa)));
            row[jB] = fma(wB, m1i, fma(Ae[i], wkb, -pc * MM(c, i, fb)));
            row[to] = wO * m1i;
          }
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j)
              S[c][i][j] += -w_minus * (Ae[j] * M1(c, i) + Ae[i] * M1(c, j)) + pc * MM(c, i, j);
        }
      } else {   // Dirichlet: SWIPDG::BoundaryLHS, penalty sigma_b kappa (n.An) / |F|^beta
        const double pc = (a.sigma_boundary * dm) * ihp;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) S[c][i][j] += -(Ae[j] * M1(c, i) + Ae[i] * M1(c, j)) + pc * MM(c, i, j);
      }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) img[c][i * rowlen + pos_self * 3 + j] = j >= i ? S[c][i][j] : S[c][j][i];
  }
};

// C3 fused: the affine part and the components of an OS2014-type diffusion factor share the phase of their
// sinusoid (kappa_c = a_c + b_c sin(kx x + ky y), problems/OS2014.hh:63-76), so one launch evaluates the 15
// sines of an element ONCE and emits every component from them: per tile, the sines (the volume sum
// sum_q w_q sin and the 3 x 3 face values) stay in registers and the component loop of the persistent
// driver builds each component's LDS image and streams it to that component's value array.  The mesh and
// the gathers are read once instead of once per component.  Entries equal the per-component kernel's up to
// rounding (kappa's volume sum is a_c sum w + b_c sum w sin instead of sum w (a_c + b_c sin)).
// TWO: exactly two components (C3), emitted in one pass over the geometry into two LDS images (emit_two)
template <int TK, bool VX = false, bool TWO_ = false>
struct P1SmoothFusedPolicy : P1SmoothPolicy<TK, VX> {
  using Base = P1SmoothPolicy<TK, VX>;
  using Own = typename Base::Own;
  using Gat = typename Base::Gat;
  static constexpr bool FUSED = true;
  static constexpr bool TWO = TWO_;
  // one wave per SIMD with the whole register file: at two (<= 256 registers) the shared sines, the tile's
  // records and the next tile's in-flight data spill (160-400 B of scratch per lane)
  static constexpr int WGCU = 4, MINW = 1;
  struct Shared {
    double sv;            // sum_q w_q sin(phase(x_q)) (Dunavant 6)
    double sf[3][3];      // sin at the Gauss 3 points of every face
  };
  __device__ static constexpr double wv()   // sum_q w_q = 1/2, the reference triangle's area
  {
    double w = 0.0;
    for (int q = 0; q < 6; ++q) w += VolRule<Simplex, 6>::w(q);
    return w;
  }
  __device__ static void prepare(const AssembleArgs& a, const Own& o, Shared& sh)
  {
    using E = Simplex;
    const KappaArg& K = a.kappa[0];   // the phase (kx, ky) every fused component shares
    const double j00 = o.X[1] - o.X[0], j01 = o.X[2] - o.X[0], j10 = o.Y[1] - o.Y[0], j11 = o.Y[2] - o.Y[0];
    sh.sv = 0.0;
    // phase = p0 + xh d1 + yh d2 on the element; when every lane's element is small against the wavelength
    // (|d1| + |d2| <= SMALL_PHASE, wave-uniform), one reduction per element (sincos of p0) and Taylor offsets
    // per point (trig_phase.hh) instead of 15 full reductions
    const double d1 = K.kx * j00 + K.ky * j10, d2 = K.kx * j01 + K.ky * j11;
    if (__all(fabs(d1) + fabs(d2) <= SMALL_PHASE)) {
      double s0, c0;
      sincos_phase(K.kx * o.X[0] + K.ky * o.Y[0], s0, c0);
#pragma unroll
      for (int q = 0; q < 6; ++q)
        sh.sv += VolRule<Simplex, 6>::w(q) * sin_near(s0, c0, VolRule<Simplex, 6>::x(q) * d1 + VolRule<Simplex, 6>::y(q) * d2);
      const double dv[3] = {0.0, d1, d2};
#pragma unroll
      for (int f = 0; f < 3; ++f) {
        const double da = dv[E::fv(f, 0)], db = dv[E::fv(f, 1)];
#pragma unroll
        for (int q = 0; q < 3; ++q) sh.sf[f][q] = sin_near(s0, c0, da + Gauss01<3>::s(q) * (db - da));
      }
      return;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const double xh = VolRule<Simplex, 6>::x(q), yh = VolRule<Simplex, 6>::y(q);
      const double x = o.X[0] + j00 * xh + j01 * yh, y = o.Y[0] + j10 * xh + j11 * yh;
      sh.sv += VolRule<Simplex, 6>::w(q) * sin_phase(K.kx * x + K.ky * y);
    }
#pragma unroll
    for (int f = 0; f < 3; ++f) {
      const int fa = E::fv(f, 0), fb = E::fv(f, 1);
      const double Ax = o.X[fa], Ay = o.Y[fa], tx = o.X[fb] - Ax, ty = o.Y[fb] - Ay;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double sq = Gauss01<3>::s(q);
        sh.sf[f][q] = sin_phase(K.kx * (Ax + sq * tx) + K.ky * (Ay + sq * ty));
      }
    }
  }
  template <bool ALLIN = false>
  __device__ static void emit_component(const AssembleArgs& a, int c, int64_t e, const Own& o, const Gat& gt,
                                        const Shared& sh, double* img)
  {
    const KappaArg& K = a.kappa[c];
    Base::template emit<ALLIN>(a, e, o, gt, img, K.c * wv() + K.b * sh.sv,
                               [&](int f, double, double, int q) { return K.c + K.b * sh.sf[f][q]; });
  }
  // both components of a two-component call in one pass over the geometry (the C3 case: OS2014's affine part and
  // its mu-component), into the images img0 / img1
  template <bool ALLIN = false>
  __device__ static void emit_two(const AssembleArgs& a, int64_t e, const Own& o, const Gat& gt, const Shared& sh,
                                  double* img0, double* img1)
  {
    const KappaArg& K0 = a.kappa[0];
    const KappaArg& K1 = a.kappa[1];
    double* const imgs[2] = {img0, img1};
    const double kvs[2] = {K0.c * wv() + K0.b * sh.sv, K1.c * wv() + K1.b * sh.sv};
    Base::template emitN<2, ALLIN>(a, e, o, gt, imgs, kvs, [&](int c, int f, double, double, int q) {
      return c == 0 ? K0.c + K0.b * sh.sf[f][q] : K1.c + K1.b * sh.sf[f][q];
    });
  }
  // (no FULLTILE path: a branch-free second copy of the two-component emission measured slower -- C3 0.249 vs 0.234
  // ms per assembly, rocprof averages on one box, profiles/r06/c_c3/; the kernel is one wave per SIMD and larger code
  // / register allocation across both copies cost more than the branches save)
};

}  // namespace dev
}  // namespace hdd
