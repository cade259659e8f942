// dune-hdd_amd/csrc/host/quadrature.cpp -- host quadrature rules and 1D Lagrange tables (quadrature.hh)
#include "quadrature.hh"

#include <algorithm>
#include <cmath>

namespace hdd {

void gauss_legendre01(int n, double* x, double* w)   // Newton on P_n, mapped to [0,1]
{
  // P_n(z) by the three-term recurrence; dp = P_n'(z)
  auto legendre = [n](double z, double& dp) {
    double p0 = 1.0, p1 = z;
    for (int k = 2; k <= n; ++k) {
      const double p2 = ((2.0 * k - 1.0) * z * p1 - (k - 1.0) * p0) / k;
      p0 = p1;
      p1 = p2;
    }
    dp = n * (z * p1 - p0) / (z * z - 1.0);
    return p1;
  };
  for (int i = 0; i < n; ++i) {
    double z = std::cos(M_PI * (i + 0.75) / (n + 0.5)), dp = 1.0;
    for (int it = 0; it < 100; ++it) {
      const double p = legendre(z, dp);
      const double dz = p / dp;
      z -= dz;
      if (std::fabs(dz) < 1e-16) {
        legendre(z, dp);   // the weight takes the derivative at the converged point
        break;
      }
    }
    x[n - 1 - i] = 0.5 * (z + 1.0);
    w[n - 1 - i] = 1.0 / ((1.0 - z * z) * dp * dp);
  }
}

void lagrange_1d(int p, int k, double x, double* v, double* d)
{
  double val = 1.0, der = 0.0;
  for (int m = 0; m <= p; ++m) {
    if (m == k) continue;
    const double den = double(k - m) / p, f = (x - double(m) / p) / den;
    der = der * f + val / den;
    val *= f;
  }
  *v = val;
  *d = der;
}

// simplex rules on the reference triangle (area 1/2): centroid (order <= 1), 3-point interior (2),
// Dunavant 6-point (3..4), collapsed Gauss-Legendre (Duffy) beyond
int simplex_rule(int order, double (*q)[4], int cap)
{
  if (order <= 1) {
    q[0][0] = q[0][1] = 1.0 / 3.0; q[0][2] = 0.0; q[0][3] = 0.5;
    return 1;
  }
  if (order == 2) {
    const double a = 1.0 / 6.0, b = 2.0 / 3.0;
    const double P[3][2] = {{a, a}, {b, a}, {a, b}};
    for (int k = 0; k < 3; ++k) { q[k][0] = P[k][0]; q[k][1] = P[k][1]; q[k][2] = 0.0; q[k][3] = 1.0 / 6.0; }
    return 3;
  }
  if (order <= 4) {
    const double a = 0.44594849091596488632, wa = 0.22338158967801146570;
    const double b = 0.091576213509770743460, wb = 0.10995174365532186764;
    const double P[6][3] = {{a, a, wa}, {1 - 2 * a, a, wa}, {a, 1 - 2 * a, wa},
                            {b, b, wb}, {1 - 2 * b, b, wb}, {b, 1 - 2 * b, wb}};
    for (int k = 0; k < 6; ++k) { q[k][0] = P[k][0]; q[k][1] = P[k][1]; q[k][2] = 0.0; q[k][3] = 0.5 * P[k][2]; }
    return 6;
  }
  const int n = (order + 3) / 2;
  if (n * n > cap) return -1;
  double s[16], w[16];
  gauss_legendre01(n, s, w);
  int k = 0;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j, ++k) {
      q[k][0] = s[i]; q[k][1] = s[j] * (1.0 - s[i]); q[k][2] = 0.0; q[k][3] = w[i] * w[j] * (1.0 - s[i]);
    }
  return n * n;
}

int tensor_rule(int dim, int order, double (*q)[4], int cap)
{
  const int n = std::max(1, (order + 2) / 2);
  int tot = 1;
  for (int a = 0; a < dim; ++a) tot *= n;
  if (tot > cap || n > 16) return -1;
  double s[16], w[16];
  gauss_legendre01(n, s, w);
  for (int m = 0; m < tot; ++m) {
    int r = m;
    q[m][0] = q[m][1] = q[m][2] = 0.0;
    q[m][3] = 1.0;
    for (int a = 0; a < dim; ++a) {
      q[m][a] = s[r % n];
      q[m][3] *= w[r % n];
      r /= n;
    }
  }
  return tot;
}

int face_rule(int fdim, int order, double (*q)[3], int cap)
{
  double t[64][4];
  const int nq = tensor_rule(fdim, order, t, std::min(cap, 64));
  for (int k = 0; k < nq; ++k) { q[k][0] = t[k][0]; q[k][1] = t[k][1]; q[k][2] = t[k][3]; }
  return nq;
}

void hex_tables(int degree, int nq1v, int nq1f, const HexTableRefs& t)
{
  gauss_legendre01(nq1v, t.sv, t.wv);
  gauss_legendre01(nq1f, t.sf, t.wf);
  for (int r = 0; r <= degree; ++r) {
    for (int q = 0; q < nq1v; ++q) lagrange_1d(degree, r, t.sv[q], &t.Lv[r][q], &t.Dv[r][q]);
    for (int q = 0; q < nq1f; ++q) lagrange_1d(degree, r, t.sf[q], &t.Lf[r][q], &t.Df[r][q]);
    for (int q = 0; q < 2; ++q) lagrange_1d(degree, r, double(q), &t.Le[r][q], &t.De[r][q]);
  }
}

}  // namespace hdd
