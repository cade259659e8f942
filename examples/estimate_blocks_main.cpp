// examples/estimate_blocks_main.cpp -- solve and localize the error on the device, through the C++ surface
// (include/hdd_discretizations.hh): the ESV2007 problem on one level of the conforming ladder of the reference's study
// (esv2007_ladder.hh), partitioned into P x P subdomains (the boxes of [-1,1]^2 the element centroids fall into),
// BlockSWIPDG::solve, then BlockSWIPDG::estimate_block for every available estimator and estimate_local_block -- the
// rows of test/linearelliptic-block-swipdg-expectations_esv2007_2daluconform.cxx:35-134 for the partitioning [P P 1].
// The efficiency divides by the energy error (kappa = 1, A = I: the H1 seminorm).
// Usage: estimate_blocks_main [level = 1] [P = 4]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <numeric>
#include <stdexcept>
#include <vector>

#include "esv2007_ladder.hh"
#include "hdd_discretizations.hh"

using namespace Dune::HDD::LinearElliptic;
using namespace esv2007;

int main(int argc, char** argv)
{
  const int level = argc > 1 ? std::atoi(argv[1]) : 1;
  const int P = argc > 2 ? std::atoi(argv[2]) : 4;
  if (level < 0 || level > 5 || P < 1 || P > 64) {
    std::printf("usage: estimate_blocks_main [level 0..5] [P 1..64]\n");
    return 1;
  }
  Mesh m = nvb_mesh(4, 2 + 2 * level);
  const size_t ne = m.ev.size() / 3;
  // the box of every element, and the elements in subdomain-major order (the order the grid keeps)
  std::vector<int32_t> box(ne);
  for (size_t e = 0; e < ne; ++e) {
    double cx = 0.0, cy = 0.0;
    for (int i = 0; i < 3; ++i) {
      cx += m.xy[2 * m.ev[3 * e + i]] / 3.0;
      cy += m.xy[2 * m.ev[3 * e + i] + 1] / 3.0;
    }
    const int ix = std::min(P - 1, std::max(0, int((cx + 1.0) / 2.0 * P))), iy = std::min(P - 1, std::max(0, int((cy + 1.0) / 2.0 * P)));
    box[e] = iy * P + ix;
  }
  std::vector<size_t> order(ne);
  std::iota(order.begin(), order.end(), size_t(0));
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return box[a] < box[b]; });
  std::vector<int32_t> ev(3 * ne), sd(ne);
  for (size_t k = 0; k < ne; ++k) {
    for (int i = 0; i < 3; ++i) ev[3 * k + i] = m.ev[3 * order[k] + i];
    sd[k] = box[order[k]];
  }
  m.ev = ev;
  hdd_grid* g = nullptr;
  if (hdd_grid_create_from_connectivity(HDD_SIMPLEX, int64_t(m.xy.size() / 2), m.xy.data(), int64_t(ne), m.ev.data(), sd.data(),
                                        P * P, HDD_BOUNDARY_ALL_DIRICHLET, &g) != HDD_OK) {
    std::printf("grid: %s\n", hdd_last_error(nullptr));
    return 1;
  }
  int rc = 0;
  try {
    Discretizations::BlockSWIPDG sw(g, Problems::ESV2007());
    sw.init();
    Discretizations::SolverOptions opt;
    opt.rtol = 1e-10;
    hdd_solve_info info{};
    const std::vector<double> u = sw.solve(0.0, opt, &info);
    std::printf("level %d: %zu triangles, %d subdomains, %zu dofs, %d iterations, residual %.3e\n", level, ne,
                sw.num_subdomains(), u.size(), info.iterations, info.residual);
    const double energy = h1_error(m, u);
    std::printf("energy error %.2e\n", energy);
    std::map<std::string, double> eta;
    for (const auto& id : sw.available_block_estimators()) eta[id] = sw.estimate_block(u, id);
    if (eta.size() != 5) rc = 2;
    for (const char* id : {"eta_NC_OS2014", "eta_R_OS2014", "eta_DF_OS2014", "eta_OS2014"}) std::printf("%s %.2e\n", id, eta[id]);
    std::printf("eff_OS2014 %.2f\n", eta["eta_OS2014"] / energy);
    std::printf("eta_R_OS2014_* %.2e\n", eta["eta_R_OS2014_*"]);
    const std::vector<double> ind = sw.estimate_local_block(u, "eta_OS2014");
    std::printf("estimate kernels %s\n", hdd_last_estimate_kernels());
    if (int(ind.size()) != sw.num_subdomains()) rc = 3;
    const size_t worst = size_t(std::max_element(ind.begin(), ind.end()) - ind.begin());
    std::printf("largest indicator %.3e in subdomain %zu of %zu\n", ind[worst], worst, ind.size());
    // kappa = 1: every factor is 1 and the indicators sum to 3 (sum N_s + sum R_s + sum D_s) / eta^2
    const auto e = sw.estimate_block_all(u, 0.0, 0.0, 0.0, 0.0, 0.0);
    const double want = 3.0 * (e.sums[0] + e.sums[1] + e.sums[2]) / e.sums[3];
    const double total = std::accumulate(ind.begin(), ind.end(), 0.0);
    std::printf("sum of estimate_local_block %.12f (3 sum / eta^2 = %.12f)\n", total, want);
    if (std::fabs(total - want) > 1e-10 * want) rc = 4;
    try {
      sw.estimate_block(u, "eta_OS2014_*");
      rc = 5;
    } catch (const Dune::Stuff::Exceptions::you_are_using_this_wrong&) {
    }
  } catch (const std::exception& e) {
    std::printf("failed: %s\n", e.what());
    rc = 6;
  }
  hdd_grid_destroy(g);
  if (rc == 0) std::printf("estimate blocks ok\n");
  return rc;
}
