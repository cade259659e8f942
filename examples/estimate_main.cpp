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
#include <string>
#include <vector>

#include "esv2007_ladder.hh"
#include "hdd_discretizations.hh"

using namespace Dune::HDD::LinearElliptic;
using namespace esv2007;

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
