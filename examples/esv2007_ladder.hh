// examples/esv2007_ladder.hh -- what the estimator examples share: the conforming ladder of the reference's ESV2007 study
// (newest-vertex bisection of the Kuhn triangulation of a 4 x 4 grid of [-1,1]^2) and the energy error of a P1 DG vector
// against the exact solution cos(pi x / 2) cos(pi y / 2).
#pragma once
#include <cmath>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace esv2007 {
struct Mesh {
  std::vector<double> xy;     // [nv][2]
  std::vector<int32_t> ev;    // [ne][3]
};

// (a, b, newest) triangles with refinement edge a-b, bisected `refines` times
inline Mesh nvb_mesh(int n0, int refines)
{
  Mesh m;
  std::map<std::pair<int64_t, int64_t>, int32_t> idx;   // coordinates in units of 2^-30 -> vertex
  auto vertex = [&](double x, double y) {
    const std::pair<int64_t, int64_t> key(std::llround(x * 1073741824.0), std::llround(y * 1073741824.0));
    auto it = idx.find(key);
    if (it != idx.end()) return it->second;
    const int32_t v = int32_t(m.xy.size() / 2);
    idx[key] = v;
    m.xy.push_back(x);
    m.xy.push_back(y);
    return v;
  };
  auto node = [&](int i, int j) { return vertex(-1.0 + 2.0 * i / n0, -1.0 + 2.0 * j / n0); };
  for (int j = 0; j <= n0; ++j)
    for (int i = 0; i <= n0; ++i) node(i, j);
  std::vector<int32_t> tri;
  for (int j = 0; j < n0; ++j)
    for (int i = 0; i < n0; ++i) {
      const int32_t v00 = node(i, j), v10 = node(i + 1, j), v01 = node(i, j + 1), v11 = node(i + 1, j + 1);
      for (int32_t v : {v00, v11, v10, v00, v11, v01}) tri.push_back(v);
    }
  for (int r = 0; r < refines; ++r) {
    std::vector<int32_t> next;
    for (size_t t = 0; t < tri.size(); t += 3) {
      const int32_t a = tri[t], b = tri[t + 1], c = tri[t + 2];
      const int32_t mid = vertex(0.5 * (m.xy[2 * a] + m.xy[2 * b]), 0.5 * (m.xy[2 * a + 1] + m.xy[2 * b + 1]));
      for (int32_t v : {a, c, mid, c, b, mid}) next.push_back(v);
    }
    tri.swap(next);
  }
  m.ev = tri;
  return m;
}

// |u - u_h|_H1 against u = cos(pi x / 2) cos(pi y / 2), 5 x 5 collapsed Gauss points per triangle (order 8)
inline double h1_error(const Mesh& m, const std::vector<double>& u)
{
  static const double gx[5] = {-0.90617984593866399280, -0.53846931010568309104, 0.0, 0.53846931010568309104,
                               0.90617984593866399280};
  static const double gw[5] = {0.23692688505618908751, 0.47862867049936646804, 0.56888888888888888889,
                               0.47862867049936646804, 0.23692688505618908751};
  const double k = 0.5 * M_PI;
  double sum = 0.0;
  for (size_t e = 0; e < m.ev.size() / 3; ++e) {
    double p[3][2];
    for (int i = 0; i < 3; ++i) {
      p[i][0] = m.xy[2 * m.ev[3 * e + i]];
      p[i][1] = m.xy[2 * m.ev[3 * e + i] + 1];
    }
    const double det = (p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[2][0] - p[0][0]) * (p[1][1] - p[0][1]);
    const double* w = &u[3 * e];
    const double g0 = (w[0] * (p[1][1] - p[2][1]) + w[1] * (p[2][1] - p[0][1]) + w[2] * (p[0][1] - p[1][1])) / det;
    const double g1 = (w[0] * (p[2][0] - p[1][0]) + w[1] * (p[0][0] - p[2][0]) + w[2] * (p[1][0] - p[0][0])) / det;
    for (int i = 0; i < 5; ++i)
      for (int j = 0; j < 5; ++j) {
        const double s = 0.5 * (gx[i] + 1.0), t = 0.5 * (gx[j] + 1.0) * (1.0 - s);
        const double wq = 0.25 * gw[i] * gw[j] * (1.0 - s);
        const double x = p[0][0] + (p[1][0] - p[0][0]) * s + (p[2][0] - p[0][0]) * t;
        const double y = p[0][1] + (p[1][1] - p[0][1]) * s + (p[2][1] - p[0][1]) * t;
        const double d0 = -k * std::sin(k * x) * std::cos(k * y) - g0, d1 = -k * std::cos(k * x) * std::sin(k * y) - g1;
        sum += std::fabs(det) * wq * (d0 * d0 + d1 * d1);
      }
  }
  return std::sqrt(sum);
}
}  // namespace esv2007
