// dune-hdd_amd/csrc/kernels/swipdg_policy_generic.hh -- the thread-per-element quadrature policy of the
// persistent tile driver (GenericPolicy: Q1, smooth coefficients on either element), the Q1 closed forms
// (Q1PwcPolicy, the C1 / C4 kernel) and the element-local products (VolProductPolicy).
#pragma once
#include <type_traits>

#include "swipdg_elements.hh"
#include "swipdg_policy.hh"

namespace hdd {
namespace dev {

// ------------------------------------------------------------------------------------------------
// Generic thread-per-element policy (Q1 parallelograms, smooth coefficients): quadrature at compile-time
// points on my side, "role" coordinates on the neighbour side.  Roles are named by physical position
// (A = my fv(f,0), B = my fv(f,1), third role = the neighbour vertex next to A off the face, fourth
// (cubes) = next to B) and numbered like the reference element, so the neighbour's basis in role
// coordinates is E::shape at the compile-time point (s, 0) and only the LDS column slots depend on the
// twin face / reversal.  Gathers per face: one neighbour vertex (2 doubles), its tensor, its kappa.
// ------------------------------------------------------------------------------------------------
template <class E>
struct GOwn {
  double X[E::NV], Y[E::NV];
  int32_t nbr[E::NF];
  uint32_t finfo;
  Tensor A;
  double ke;
  int32_t vid[E::NV];   // VX: local vertex ids (as P1Own)
};
template <class E>
struct GGat {
  double Cx[E::NF], Cy[E::NF];
  Tensor Ap[E::NF];
  double kn[E::NF];
  int32_t ov[E::NF];    // VX: the neighbour's third-role vertex id
};

template <class E, int NQV, int NQF, int TK, int KK, bool VX = false>
struct GenericPolicy : PolicyDefaults {
  static constexpr int NB = E::NB, NF = E::NF, NV = E::NV;
  static constexpr int RB = (NF + 1) * NB * NB;
  // workgroups (single-wave tiles) per CU and the register cap: simplices (18 KB tiles) run 8 per CU at
  // <= 256 registers (2 waves / SIMD hide the sinusoid's VALU latency: C3 0.278 -> 0.241 ms per component,
  // profiles/r01/s2/ab1.log); quads are LDS-bound at 4 per CU (40 KB rotated image) and keep the full
  // register file (capping them at 256 spills: 0.84 -> 1.30 ms)
  static constexpr int WGCU = NB == 4 ? 4 : 8;
  static constexpr int MINW = NB == 4 ? 1 : 2;
  static constexpr bool PAD = NB == 4;   // rotated LDS image for uniform tiles (see the persistent kernel)
  using Own = GOwn<E>;
  using Gat = GGat<E>;

  __device__ static void load_own(const AssembleArgs& a, int64_t e, Own& o)
  {
    const int64_t ne = a.n_local;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      if constexpr (VX) {
        o.vid[k] = a.ev[k * ne + e];
      } else {
        o.X[k] = a.coords[(2 * k) * ne + e];
        o.Y[k] = a.coords[(2 * k + 1) * ne + e];
      }
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) o.nbr[f] = a.nbrs[f * ne + e];
    o.finfo = a.finfo[e];
    o.A = tensor_k<TK>(a, e);
    o.ke = smooth_kind(KK) ? 0.0 : kappa_k<KK == HDD_FN_PER_ELEM ? HDD_FN_PER_ELEM : HDD_FN_CONST>(a, e);
  }

  __device__ static void load_gat(const AssembleArgs& a, int64_t e, Own& o, Gat& g)
  {
    const int64_t ne = a.n_local;
    if constexpr (VX) {
#pragma unroll
      for (int k = 0; k < NV; ++k) vertex_xy(a, o.vid[k], o.X[k], o.Y[k]);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int64_t n = o.nbr[f] >= 0 ? int64_t(o.nbr[f]) : e;
      const int c = role_slot<E>(o.finfo, f, 2);
      if constexpr (VX) {
        g.ov[f] = a.ev[c * ne + n];
      } else {
        g.Cx[f] = a.coords[(2 * c) * ne + n];
        g.Cy[f] = a.coords[(2 * c + 1) * ne + n];
      }
      g.Ap[f] = tensor_k<TK>(a, n);
      g.kn[f] = smooth_kind(KK) ? 0.0 : kappa_k<KK == HDD_FN_PER_ELEM ? HDD_FN_PER_ELEM : HDD_FN_CONST>(a, n);
    }
  }

  __device__ static void load_gat2(const AssembleArgs& a, Gat& g)
  {
    if constexpr (VX) {
#pragma unroll
      for (int f = 0; f < NF; ++f) vertex_xy(a, g.ov[f], g.Cx[f], g.Cy[f]);
    }
  }

  __device__ static double kap(const AssembleArgs& a, double x, double y)
  {
    const KappaArg& K = a.kappa[0];
    if constexpr (KK == HDD_FN_FLATTOP) return flattop_sum(K.table, K.n_table, K.c, K.b, x, y);
    return K.c + K.b * sin_phase(K.kx * x + K.ky * y);
  }

  __device__ static int n_interior(const Own& o)
  {
    int c = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f) c += o.nbr[f] >= 0;
    return c;
  }

  template <class IMG>
  __device__ static void compute(const AssembleArgs& a, int64_t e, const Own& o, const Gat& gt, IMG img)
  {
    Geom G;
    G.init(o.X[0], o.Y[0], o.X[1], o.Y[1], o.X[2], o.Y[2]);
    const double adet = fabs(G.det);
    const double osgn = G.det > 0.0 ? 1.0 : -1.0;
    int pos_self = 0, pos[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) pos_self += (o.nbr[f] >= 0 && o.nbr[f] < e);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      int p = (e < o.nbr[f]) ? 1 : 0;
#pragma unroll
      for (int q = 0; q < NF; ++q) p += (o.nbr[q] >= 0 && o.nbr[q] < o.nbr[f]);
      pos[f] = p;
    }
    const int rowlen = (n_interior(o) + 1) * NB;
    double S[NB][NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) S[i][j] = 0.0;
    // ---- LocalEvaluation::Elliptic ----
#pragma unroll
    for (int q = 0; q < NQV; ++q) {
      double phi[NB], ghx[NB], ghy[NB], gx[NB], gy[NB];
      E::shape(VolRule<E, NQV>::x(q), VolRule<E, NQV>::y(q), phi, ghx, ghy);
#pragma unroll
      for (int k = 0; k < NB; ++k) G.grad(ghx[k], ghy[k], gx[k], gy[k]);
      double kq = o.ke;
      if constexpr (smooth_kind(KK)) {
        double px, py;
        G.global(VolRule<E, NQV>::x(q), VolRule<E, NQV>::y(q), px, py);
        kq = kap(a, px, py);
      }
      const double fac = VolRule<E, NQV>::w(q) * adet * kq;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const double Agx = o.A.a00 * gx[j] + o.A.a01 * gy[j];
        const double Agy = o.A.a01 * gx[j] + o.A.a11 * gy[j];
#pragma unroll
        for (int i = 0; i < NB; ++i) S[i][j] += fac * (Agx * gx[i] + Agy * gy[i]);
      }
    }
    // ---- faces ----
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int32_t n = o.nbr[f];
      if (n <= HDD_NBR_NEUMANN) continue;
      const int fa = E::fv(f, 0), fb = E::fv(f, 1);
      const double Ax = o.X[fa], Ay = o.Y[fa], Bx = o.X[fb], By = o.Y[fb];
      const double tx = Bx - Ax, ty = By - Ay;
      const double il = rsq_nr(tx * tx + ty * ty);
      const double len = (tx * tx + ty * ty) * il;
      const double nsc = E::face_sign(f) * osgn * il;
      const double nx = ty * nsc, ny = -tx * nsc;
      const double dm = agn(o.A, nx, ny, nx, ny);
      const double ihp = a.beta == 1.0 ? il : inv_pow(len, a.beta);
      const double rax = E::rv(fa, 0), ray = E::rv(fa, 1), rbx = E::rv(fb, 0), rby = E::rv(fb, 1);
      if (n >= 0) {
        Geom Hn;   // neighbour in role coordinates: A = (0,0), B = (1,0), third role = (0,1)
        Hn.init(Ax, Ay, Bx, By, gt.Cx[f], gt.Cy[f]);
        const Tensor Ap = gt.Ap[f];
        const double dp = agn(Ap, nx, ny, nx, ny);
        const double rs = rcp_nr(dp + dm);
        const double gamma = (dp * dm) * rs;
        const double w_plus = dm * rs, w_minus = dp * rs;
        double EN[NB][NB];
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int j = 0; j < NB; ++j) EN[i][j] = 0.0;
#pragma unroll
        for (int q = 0; q < NQF; ++q) {
          const double s = Gauss01<NQF>::s(q);
          double pe[NB], ghx[NB], ghy[NB], gex[NB], gey[NB];
          E::shape(rax + s * (rbx - rax), ray + s * (rby - ray), pe, ghx, ghy);
#pragma unroll
          for (int k = 0; k < NB; ++k) G.grad(ghx[k], ghy[k], gex[k], gey[k]);
          double pn[NB], hhx[NB], hhy[NB];
          E::shape(s, 0.0, pn, hhx, hhy);
          double kme = o.ke, knb = gt.kn[f];
          if constexpr (smooth_kind(KK)) {
            kme = kap(a, Ax + s * tx, Ay + s * ty);
            knb = kme;
          }
          const double pen = (kme * knb * a.sigma_inner * gamma) * ihp;
          const double fac = Gauss01<NQF>::w(q) * len;
          double Ae[NB], An[NB];
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            double hx, hy;
            Hn.grad(hhx[k], hhy[k], hx, hy);
            Ae[k] = agn(o.A, gex[k], gey[k], nx, ny);
            An[k] = agn(Ap, hx, hy, nx, ny);
          }
#pragma unroll
          for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
              S[i][j] += fac * (-w_minus * kme * Ae[j] * pe[i] - w_minus * kme * pe[j] * Ae[i] + pen * pe[j] * pe[i]);
              EN[i][j] += fac * (-w_plus * knb * An[j] * pe[i] + w_minus * kme * pn[j] * Ae[i] - pen * pn[j] * pe[i]);
            }
        }
        int slot[NB];
#pragma unroll
        for (int r = 0; r < NB; ++r) slot[r] = role_slot<E>(o.finfo, f, r);
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
          for (int r = 0; r < NB; ++r) img[i * rowlen + pos[f] * NB + slot[r]] = EN[i][r];
      } else {   // Dirichlet: SWIPDG::BoundaryLHS
#pragma unroll
        for (int q = 0; q < NQF; ++q) {
          const double s = Gauss01<NQF>::s(q);
          double pe[NB], ghx[NB], ghy[NB], gex[NB], gey[NB];
          E::shape(rax + s * (rbx - rax), ray + s * (rby - ray), pe, ghx, ghy);
#pragma unroll
          for (int k = 0; k < NB; ++k) G.grad(ghx[k], ghy[k], gex[k], gey[k]);
          double kme = o.ke;
          if constexpr (smooth_kind(KK)) kme = kap(a, Ax + s * tx, Ay + s * ty);
          const double pen = (a.sigma_boundary * kme * dm) * ihp;
          const double fac = Gauss01<NQF>::w(q) * len;
          double Ae[NB];
#pragma unroll
          for (int k = 0; k < NB; ++k) Ae[k] = agn(o.A, gex[k], gey[k], nx, ny);
#pragma unroll
          for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j)
              S[i][j] += fac * (-kme * Ae[j] * pe[i] - kme * pe[j] * Ae[i] + pen * pe[j] * pe[i]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) img[i * rowlen + pos_self * NB + j] = S[i][j];
  }
};

// ------------------------------------------------------------------------------------------------
// Q1 on parallelograms, piecewise-constant coefficients: closed-form face integrals.
//
// On an affine quadrilateral the trace of a Q1 function on a face is linear in the face parameter s and
// so is (A grad phi) . n, so every face integrand of SWIPDG::Inner / BoundaryLHS is a quadratic in s: the
// reference's 2-point Gauss rule integrates it exactly, and so does the closed form used here,
//   int (A grad phi_j . n) phi_i = |F| (p_i alpha_j + q_i beta_j),  int phi_i phi_j = |F| M_ij,
// with alpha_j / beta_j the values at the face's first / second vertex, (p, q) = (1/3, 1/6) for the first
// face vertex and (1/6, 1/3) for the second, M = [[1/3, 1/6], [1/6, 1/3]] on the face vertices.  The
// vertex values are ghat_j(v) . m with m = J^{-1} A n (one 2-vector per face and side) and the reference
// gradients ghat_j(v) compile-time constants in {0, +-1}.  The volume term keeps the reference's 1-point
// rule (integrand order 0 for piecewise-constant data): S_ij = |det J| kappa ghat_i(c)^T J^{-1} A J^{-T}
// ghat_j(c).  Results equal the quadrature form up to rounding (GPU parity tolerance 1e-12 of the row
// maximum).  Neighbour quantities are in role coordinates (A = my face vertex a, B = b, C = the
// neighbour vertex next to A), as in GenericPolicy.
// ------------------------------------------------------------------------------------------------
// PEN: penalty terms only (the SWIPDG penalty product).  H2: half images (see the persistent kernel): the tile's
// two 32-element halves are computed and streamed in turn through a 20 KB image, so 8 tiles fit per CU and the
// kernel runs two waves per SIMD (<= 256 registers) instead of one.
template <int TK, int KK, bool PEN = false, bool VX = false, bool H2 = false>
struct Q1PwcPolicy : GenericPolicy<Cube, 1, 2, TK, KK, VX> {
  using Base = GenericPolicy<Cube, 1, 2, TK, KK, VX>;
  using E = Cube;
  static constexpr int NB = 4, NF = 4;
  static constexpr bool HALF = H2;
  static constexpr bool EMIT = true;   // emit(): the row block one 4 x 4 block at a time (the sharded SoA fixup)
  static constexpr int WGCU = H2 ? 8 : 4, MINW = H2 ? 2 : 1;
  using Own = typename Base::Own;
  using Gat = typename Base::Gat;

  // reference Q1 gradient of basis k at the reference point (x, y): component d
  __host__ __device__ static constexpr double gh(int k, int d, double x, double y)
  {
    return d == 0 ? ((k & 1) ? 1.0 : -1.0) * ((k & 2) ? y : 1.0 - y)
                  : ((k & 2) ? 1.0 : -1.0) * ((k & 1) ? x : 1.0 - x);
  }

  // Canonical register order of one element's values: V[i * VR + b * NB + c], row i, block b (0: the element
  // itself, column c = basis j; 1 + f: the neighbour across face f, column c = role r).  VR = 20 values per row.
  static constexpr int VR = (NF + 1) * NB, NV80 = NB * VR;

  // block positions inside the element's row block (blocks sorted by element id): the element's own, face f's
  __device__ static void positions(int64_t e, const Own& o, int& pos_self, int* pos)
  {
    pos_self = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f) pos_self += (o.nbr[f] >= 0 && o.nbr[f] < e);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      int p = (e < o.nbr[f]) ? 1 : 0;
#pragma unroll
      for (int q = 0; q < NF; ++q) p += (o.nbr[q] >= 0 && o.nbr[q] < o.nbr[f]);
      pos[f] = p;
    }
  }

  // the element's row block into an LDS image (row length (1 + interior faces) * NB, blocks sorted by element id)
  template <class IMG>
  __device__ static void compute(const AssembleArgs& a, int64_t e, const Own& o, const Gat& gt, IMG img)
  {
    int pos_self, pos[NF];
    positions(e, o, pos_self, pos);
    const int rowlen = (Base::n_interior(o) + 1) * NB;
    emit(a, o, gt, [&](int b, const double (&blk)[NB][NB]) {
      if (b > 0 && o.nbr[b - 1] < 0) return;
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int c = 0; c < NB; ++c)
          img[i * rowlen + (b == 0 ? pos_self * NB + c : pos[b - 1] * NB + role_slot<E>(o.finfo, b - 1, c))] = blk[i][c];
    });
  }

  // The closed forms.  sink(b, blk) receives the row block one 4 x 4 block at a time, blk[i][c] = row i, column c: the
  // neighbour blocks face by face (b = 1 + f, column c = role r; called for every face in uniform control flow,
  // zeros when face f has no neighbour), the element's own block last (b = 0, column c = basis j).
  template <class SINK>
  __device__ static void emit(const AssembleArgs& a, const Own& o, const Gat& gt, SINK&& sink)
  {
    const double j00 = o.X[1] - o.X[0], j01 = o.X[2] - o.X[0], j10 = o.Y[1] - o.Y[0], j11 = o.Y[2] - o.Y[0];
    const double det = j00 * j11 - j01 * j10;
    const double id = rcp_nr(det);
    const double i00 = j11 * id, i01 = -j01 * id, i10 = -j10 * id, i11 = j00 * id;   // J^{-1}
    const double adet = fabs(det);
    const double osgn = det > 0.0 ? 1.0 : -1.0;
    const Tensor A = o.A;
    const double ke = o.ke;
    double S[NB][NB];
    {   // LocalEvaluation::Elliptic, 1-point rule: K = J^{-1} A J^{-T}
      const double p00 = i00 * A.a00 + i01 * A.a01, p01 = i00 * A.a01 + i01 * A.a11;
      const double p10 = i10 * A.a00 + i11 * A.a01, p11 = i10 * A.a01 + i11 * A.a11;
      const double k00 = p00 * i00 + p01 * i01, k01 = p00 * i10 + p01 * i11, k11 = p10 * i10 + p11 * i11;
      const double fac = PEN ? 0.0 : adet * ke;
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const double gix = gh(i, 0, 0.5, 0.5), giy = gh(i, 1, 0.5, 0.5);
          const double gjx = gh(j, 0, 0.5, 0.5), gjy = gh(j, 1, 0.5, 0.5);
          S[i][j] = fac * (gix * (k00 * gjx + k01 * gjy) + giy * (k01 * gjx + k11 * gjy));
        }
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int32_t n = o.nbr[f];
      double EN[NB][NB];
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int r = 0; r < NB; ++r) EN[i][r] = 0.0;
      if (n > HDD_NBR_NEUMANN) {
        const int fa = E::fv(f, 0), fb = E::fv(f, 1);
        const double ax = E::rv(fa, 0), ay = E::rv(fa, 1), bx = E::rv(fb, 0), by = E::rv(fb, 1);
        const double Ax = o.X[fa], Ay = o.Y[fa], Bx = o.X[fb], By = o.Y[fb];
        const double tx = Bx - Ax, ty = By - Ay;
        const double il = rsq_nr(tx * tx + ty * ty);
        const double len = (tx * tx + ty * ty) * il;
        const double nsc = E::face_sign(f) * osgn * il;
        const double nx = ty * nsc, ny = -tx * nsc;
        const double anx = A.a00 * nx + A.a01 * ny, any = A.a01 * nx + A.a11 * ny;
        const double dm = anx * nx + any * ny;
        const double ihp = a.beta == 1.0 ? il : inv_pow(len, a.beta);
        const double mx = i00 * anx + i01 * any, my = i10 * anx + i11 * any;   // J^{-1} A n
        double al[NB], be[NB];   // (A grad phi_k . n) at my face vertices a, b
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          al[k] = gh(k, 0, ax, ay) * mx + gh(k, 1, ax, ay) * my;
          be[k] = gh(k, 0, bx, by) * mx + gh(k, 1, bx, by) * my;
        }
        const double L3 = len * (1.0 / 3.0), L6 = len * (1.0 / 6.0);
        // int (A grad phi_j . n) phi_i  and  int phi_i phi_j
        auto I1 = [&](int j, int i) { return i == fa ? L3 * al[j] + L6 * be[j] : (i == fb ? L6 * al[j] + L3 * be[j] : 0.0); };
        auto MM = [&](int i, int j) {
          return (i == fa || i == fb) && (j == fa || j == fb) ? (i == j ? L3 : L6) : 0.0;
        };
        if (n >= 0) {
          const double Cx = gt.Cx[f], Cy = gt.Cy[f];
          const Tensor Ap = gt.Ap[f];
          const double kn = gt.kn[f];
          // neighbour in role coordinates: A = (0,0), B = (1,0), C = (0,1)
          const double h00 = Bx - Ax, h01 = Cx - Ax, h10 = By - Ay, h11 = Cy - Ay;
          const double hid = rcp_nr(h00 * h11 - h01 * h10);
          const double anpx = Ap.a00 * nx + Ap.a01 * ny, anpy = Ap.a01 * nx + Ap.a11 * ny;
          const double dp = anpx * nx + anpy * ny;
          const double mpx = (h11 * anpx - h01 * anpy) * hid, mpy = (-h10 * anpx + h00 * anpy) * hid;
          double alp[NB], bep[NB];   // (A+ grad phi+_r . n) at A (0,0) and B (1,0)
#pragma unroll
          for (int r = 0; r < NB; ++r) {
            alp[r] = gh(r, 0, 0.0, 0.0) * mpx + gh(r, 1, 0.0, 0.0) * mpy;
            bep[r] = gh(r, 0, 1.0, 0.0) * mpx + gh(r, 1, 1.0, 0.0) * mpy;
          }
          const double rs = rcp_nr(dp + dm);
          const double gamma = (dp * dm) * rs;
          const double w_plus = dm * rs, w_minus = dp * rs;
          const double pen = (ke * kn * a.sigma_inner * gamma) * ihp;
          constexpr double CS = PEN ? 0.0 : 1.0;
          const double cs = -w_minus * ke * CS, cp = -w_plus * kn * CS, cm = w_minus * ke * CS;
#pragma unroll
          for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) S[i][j] += cs * (I1(j, i) + I1(i, j)) + pen * MM(i, j);
#pragma unroll
          for (int i = 0; i < NB; ++i) {
            // int phi+_r phi_i: phi+_A = 1 - s, phi+_B = s (roles 0, 1); int phi+_r (A grad phi_i . n) likewise
            const double pi = i == fa ? L3 : (i == fb ? L6 : 0.0), qi = i == fa ? L6 : (i == fb ? L3 : 0.0);
#pragma unroll
            for (int r = 0; r < NB; ++r) {
              const double anr = pi * alp[r] + qi * bep[r];
              const double ai = r == 0 ? L3 * al[i] + L6 * be[i] : (r == 1 ? L6 * al[i] + L3 * be[i] : 0.0);
              const double mr = r == 0 ? pi : (r == 1 ? qi : 0.0);
              EN[i][r] = cp * anr + cm * ai - pen * mr;
            }
          }
        } else {   // Dirichlet: SWIPDG::BoundaryLHS
          const double pen = (a.sigma_boundary * ke * dm) * ihp;
#pragma unroll
          for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) S[i][j] += -ke * (PEN ? 0.0 : 1.0) * (I1(j, i) + I1(i, j)) + pen * MM(i, j);
        }
      }   // a neighbour or Dirichlet
      sink(1 + f, EN);
    }
    sink(0, S);
  }
};

// ------------------------------------------------------------------------------------------------
// Element-local products on the element-diagonal (volume) pattern (swipdg.hh:358-461: L2, H1Semi,
// Elliptic, BoundaryL2 with over_integrate = 2), P1 triangles / Q1 parallelograms, piecewise-constant
// data.  The reference's rules (orders 2p + 2, 2(p-1) + 2 [+ ord kappa]) integrate these polynomial
// integrands exactly, so the closed forms below equal them up to rounding:
//   P1:  l2 |det| (1 + d_ij) / 24;  h1 / elliptic  (|det| / 2) ghat_i^T K ghat_j
//   Q1:  l2 |det| M(i0,j0) M(i1,j1);  h1 / elliptic  sum_ab K_ab F^ab(i,j) with the 1D integrals
//        M = int L_i L_j, D = int L_i' L_j', C = int L_i' L_j (F^00 = D x M, F^01 = C x C^T, F^10 = C^T x C,
//        F^11 = M x D);  K = |det J| kappa J^-1 A J^-T (A = I for h1)
//   boundary l2: sum over boundary faces of |F| (1/3, 1/6) on the face vertices.
// Row block = nb x nb (no neighbour blocks), so tiles are 64 nb^2 doubles and no gathers are needed.
// ------------------------------------------------------------------------------------------------
template <class E, int KIND, int TK, int KK, int VX = 0>   // VX: vertex-indexed geometry (P1 / Q1 kernels' VX)
struct VolProductPolicy : PolicyDefaults {
  static constexpr int NB = E::NB, NF = E::NF, NV = E::NV;
  static constexpr int RB = NB * NB;
  static constexpr int WGCU = 4, MINW = 1;
  static constexpr bool PAD = false;
  struct Own {
    double X[NV], Y[NV];
    int32_t nbr[NF];
    Tensor A;
    double ke;
    int32_t vid[NV];
  };
  struct Gat {};
  static constexpr int NVL = KIND == HDD_PRODUCT_BOUNDARY_L2 ? NV : 3;   // vertices read (0, 1, 2 span the map)
  __device__ static void load_own(const AssembleArgs& a, int64_t e, Own& o)
  {
    const int64_t ne = a.n_local;
#pragma unroll
    for (int k = 0; k < NVL; ++k) {
      if constexpr (VX != 0) {
        o.vid[k] = a.ev[k * ne + e];
      } else {
        o.X[k] = a.coords[(2 * k) * ne + e];
        o.Y[k] = a.coords[(2 * k + 1) * ne + e];
      }
    }
    if constexpr (KIND == HDD_PRODUCT_BOUNDARY_L2) {
#pragma unroll
      for (int f = 0; f < NF; ++f) o.nbr[f] = a.nbrs[f * ne + e];
    }
    if constexpr (KIND == HDD_PRODUCT_ELLIPTIC) {
      o.A = tensor_k<TK>(a, e);
      o.ke = kappa_k<KK>(a, e);
    }
  }
  __device__ static void load_gat(const AssembleArgs& a, int64_t, Own& o, Gat&)
  {
    if constexpr (VX != 0) {
#pragma unroll
      for (int k = 0; k < NVL; ++k) vertex_xy(a, o.vid[k], o.X[k], o.Y[k]);
    }
  }
  __device__ static void load_gat2(const AssembleArgs&, Gat&) {}
  __device__ static int n_interior(const Own&) { return 0; }

  __host__ __device__ static constexpr double m1(int i, int j) { return i == j ? 1.0 / 3.0 : 1.0 / 6.0; }
  __host__ __device__ static constexpr double d1(int i, int j) { return i == j ? 1.0 : -1.0; }
  __host__ __device__ static constexpr double c1(int i, int) { return i ? 0.5 : -0.5; }   // int L_i' L_j

  __device__ static void compute(const AssembleArgs&, int64_t, const Own& o, const Gat&, double* img)
  {
    const double j00 = o.X[1] - o.X[0], j01 = o.X[2] - o.X[0], j10 = o.Y[1] - o.Y[0], j11 = o.Y[2] - o.Y[0];
    const double det = j00 * j11 - j01 * j10;
    const double adet = fabs(det);
    double S[NB][NB];
    if constexpr (KIND == HDD_PRODUCT_L2) {
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
          S[i][j] = std::is_same<E, Simplex>::value ? adet * (i == j ? 1.0 / 12.0 : 1.0 / 24.0)
                                                     : adet * (m1(i & 1, j & 1) * m1(i >> 1, j >> 1));
    } else if constexpr (KIND == HDD_PRODUCT_BOUNDARY_L2) {
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) S[i][j] = 0.0;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if (o.nbr[f] >= 0) continue;
        const int fa = E::fv(f, 0), fb = E::fv(f, 1);
        const double tx = o.X[fb] - o.X[fa], ty = o.Y[fb] - o.Y[fa];
        const double len = sqrt(tx * tx + ty * ty);
        S[fa][fa] += len * (1.0 / 3.0);
        S[fb][fb] += len * (1.0 / 3.0);
        S[fa][fb] += len * (1.0 / 6.0);
        S[fb][fa] += len * (1.0 / 6.0);
      }
    } else {   // H1_SEMI / ELLIPTIC: K = |det| kappa J^-1 A J^-T
      const double id = rcp_nr(det);
      const double i00 = j11 * id, i01 = -j01 * id, i10 = -j10 * id, i11 = j00 * id;
      double a00 = 1.0, a01 = 0.0, a11 = 1.0, fac = adet;
      if constexpr (KIND == HDD_PRODUCT_ELLIPTIC) {
        a00 = o.A.a00; a01 = o.A.a01; a11 = o.A.a11;
        fac *= o.ke;
      }
      const double p00 = i00 * a00 + i01 * a01, p01 = i00 * a01 + i01 * a11;
      const double p10 = i10 * a00 + i11 * a01, p11 = i10 * a01 + i11 * a11;
      const double k00 = fac * (p00 * i00 + p01 * i01), k01 = fac * (p00 * i10 + p01 * i11);
      const double k11 = fac * (p10 * i10 + p11 * i11);
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          if constexpr (std::is_same<E, Simplex>::value) {
            const double gix = i == 1 ? 1.0 : (i == 0 ? -1.0 : 0.0), giy = i == 2 ? 1.0 : (i == 0 ? -1.0 : 0.0);
            const double gjx = j == 1 ? 1.0 : (j == 0 ? -1.0 : 0.0), gjy = j == 2 ? 1.0 : (j == 0 ? -1.0 : 0.0);
            S[i][j] = 0.5 * (gix * (k00 * gjx + k01 * gjy) + giy * (k01 * gjx + k11 * gjy));
          } else {
            const int i0 = i & 1, i1 = i >> 1, jj0 = j & 1, jj1 = j >> 1;
            S[i][j] = k00 * d1(i0, jj0) * m1(i1, jj1) + k01 * c1(i0, jj0) * c1(jj1, i1) +
                      k01 * c1(jj0, i0) * c1(i1, jj1) + k11 * m1(i0, jj0) * d1(i1, jj1);
          }
        }
    }
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) img[i * NB + j] = S[i][j];
  }
};

}  // namespace dev
}  // namespace hdd
