// examples/estimate_main.cpp -- solve and certify on the device, through the C++ surface (include/hdd_discretizations.hh):
// the ESV2007 problem on one level of the conforming ladder of the reference's study (newest-vertex bisection of the
// Kuhn triangulation of a 4 x 4 grid of [-1,1]^2, 2 + 2 level bisections: 128, 512, 2048, 8192 triangles), SWIPDG::solve,
// then SWIPDG::estimate for every available estimator -- the seven estimator rows of
// test/linearelliptic-swipdg-expectations_esv2007_2daluconform.cxx:38-57.  The efficiencies divide by the energy error
// (kappa = 1, A = I: the H1 seminorm) against the exact solution cos(pi x / 2) cos(pi y / 2).
// Usage: estimate_main [level = 1]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <utility>
#include <vector>

#include "hdd_discretizations.hh"

using namespace Dune::HDD::LinearElliptic;

namespace {
struct Mesh {
  std::vector<double> xy;     // [nv][2]
  std::vector<int32_t> ev;    // [ne][3]
};

// (a, b, newest) triangles with refinement edge a-b, bisected `refines` times
Mesh nvb_mesh(int n0, int refines)
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
double h1_error(const Mesh& m, const std::vector<double>& u)
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
}  // namespace

int main(int argc, char** argv)
{
  const int level = argc > 1 ? std::atoi(argv[1]) : 1;
  if (level < 0 || level > 5) {
    std::printf("usage: estimate_main [level 0..5]\n");
    return 1;
  }
  const Mesh m = nvb_mesh(4, 2 + 2 * level);
  hdd_grid* g = nullptr;
  if (hdd_grid_create_from_connectivity(HDD_SIMPLEX, int64_t(m.xy.size() / 2), m.xy.data(), int64_t(m.ev.size() / 3),
                                        m.ev.data(), nullptr, 1, HDD_BOUNDARY_ALL_DIRICHLET, &g) != HDD_OK) {
    std::printf("grid: %s\n", hdd_last_error(nullptr));
    return 1;
  }
  int rc = 0;
  try {
    Discretizations::SWIPDG sw(g, Problems::ESV2007());
    sw.init();
    Discretizations::SolverOptions opt;
    opt.rtol = 1e-10;
    hdd_solve_info info{};
    const std::vector<double> u = sw.solve(0.0, opt, &info);
    std::printf("level %d: %zu triangles, %zu dofs, %d iterations, residual %.3e\n", level, m.ev.size() / 3, u.size(),
                info.iterations, info.residual);
    const double energy = h1_error(m, u);
    std::printf("energy error %.2e\n", energy);
    std::map<std::string, double> eta;
    for (const auto& id : sw.available_estimators()) eta[id] = sw.estimate(u, id);
    std::printf("estimate kernels %s\n", hdd_last_estimate_kernels());
    if (eta.size() != 6) rc = 2;
    for (const char* id : {"eta_NC_ESV2007", "eta_R_ESV2007", "eta_DF_ESV2007", "eta_ESV2007"})
      std::printf("%s %.2e\n", id, eta[id]);
    std::printf("eff_ESV2007 %.2f\n", eta["eta_ESV2007"] / energy);
    std::printf("eta_ESV2007_alt %.2e\n", eta["eta_ESV2007_alt"]);
    std::printf("eff_ESV2007_alt %.2f\n", eta["eta_ESV2007_alt"] / energy);
    std::printf("eta_R_ESV2007_* %.2e\n", eta["eta_R_ESV2007_*"]);
    // the local indicators sum to one
    double total = 0.0;
    for (double v : sw.estimate_local(u, "eta_ESV2007")) total += v;
    std::printf("sum of estimate_local %.12f\n", total);
    if (std::fabs(total - 1.0) > 1e-10) rc = 3;
  } catch (const std::exception& e) {
    std::printf("failed: %s\n", e.what());
    rc = 4;
  }
  hdd_grid_destroy(g);
  if (rc == 0) std::printf("estimate ok\n");
  return rc;
}
