// examples/solve_blocks_main.cpp -- the local problems of every subdomain in one device solve, through the C++ surface
// (include/hdd_discretizations.hh): ESV2007 on the 32 x 32 Q1 grid in 4 x 4 subdomains, BlockSWIPDG::solve_locals on
// the 16 local right-hand sides at once (hdd_operator_solve_blocks: three launches per iteration for all of them).
// Every subdomain must be, byte for byte, what solve_local(ss, ...) gives for it, and apply_local_operators what
// apply_local_operator(ss, ...) gives: the program exits non-zero otherwise.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "hdd_discretizations.hh"

using namespace Dune::HDD::LinearElliptic;

namespace {
bool same_bytes(const double* a, const std::vector<double>& b) { return std::memcmp(a, b.data(), b.size() * sizeof(double)) == 0; }

bool same_info(const hdd_solve_info& a, const hdd_solve_info& b)
{
  return a.status == b.status && a.iterations == b.iterations && std::memcmp(&a.residual, &b.residual, sizeof(double)) == 0 &&
         std::memcmp(&a.rhs_norm, &b.rhs_norm, sizeof(double)) == 0;
}
}  // namespace

int main()
{
  hdd_grid* g = nullptr;
  hdd_structured_desc d{HDD_CUBE, 32, 32, 4, 4, HDD_BOUNDARY_ALL_DIRICHLET, 0, {-1.0, -1.0}, {1.0, 1.0}};
  if (hdd_grid_create_structured(&d, &g) != HDD_OK) return 1;
  int rc = 0;
  try {
    Problems::Problem esv;   // kappa = 1 (affine part), A = I
    esv.force = Problems::ScalarFunction::cos_product(0.5 * M_PI * M_PI, 0.5 * M_PI, 0.5 * M_PI, 0.0, 3);
    Discretizations::BlockSWIPDG block(g, esv);
    block.init();
    const int n = block.num_subdomains();
    const std::vector<int64_t> bounds = block.subdomain_bounds();
    // the local functionals one behind the other are the global right-hand side
    const std::vector<double> b = block.rhs().affine_part();
    if (n != 16 || int64_t(b.size()) != bounds.back()) throw std::runtime_error("16 subdomains expected");
    std::vector<hdd_solve_info> infos;
    const auto x = block.solve_locals(b, 0.0, Discretizations::SolverOptions(), &infos);
    std::printf("solve kernels %s\n", hdd_last_solve_kernels());
    if (std::string(hdd_last_solve_kernels()).find("cg_direction_blocks") == std::string::npos) rc = 2;
    const auto y = block.apply_local_operators(x);
    std::printf("apply kernel %s\n", hdd_last_apply_kernel());
    if (std::string(hdd_last_apply_kernel()).find("_blocks_kernel") == std::string::npos) rc = 2;
    for (int ss = 0; ss < n; ++ss) {
      const size_t lo = size_t(bounds[size_t(ss)]), hi = size_t(bounds[size_t(ss) + 1]);
      const std::vector<double> bs(b.begin() + int64_t(lo), b.begin() + int64_t(hi));
      hdd_solve_info one{};
      const auto xs = block.solve_local(ss, bs, 0.0, Discretizations::SolverOptions(), &one);
      const auto ys = block.apply_local_operator(ss, xs);
      const bool same = xs.size() == hi - lo && same_bytes(x.data() + lo, xs) && same_info(one, infos[size_t(ss)]) &&
                        ys.size() == hi - lo && same_bytes(y.data() + lo, ys);
      std::printf("%s: subdomain %d, %d iterations, residual %.3e, ||b|| %.3e, %s the local solve\n",
                  infos[size_t(ss)].status == HDD_SOLVE_CONVERGED ? "converged" : "NOT converged", ss, infos[size_t(ss)].iterations,
                  infos[size_t(ss)].residual, infos[size_t(ss)].rhs_norm, same ? "bit-identical to" : "DIFFERS from");
      if (infos[size_t(ss)].status != HDD_SOLVE_CONVERGED || !(infos[size_t(ss)].residual <= 1e-8 * infos[size_t(ss)].rhs_norm) || !same) rc = 3;
    }
    // max_iter too small: the reference's linear-solver exception names the first subdomain that failed
    Discretizations::SolverOptions few;
    few.max_iter = 2;
    try {
      block.solve_locals(b, 0.0, few);
      std::printf("max_iter = 2 unexpectedly converged\n");
      rc = 4;
    } catch (const Dune::Stuff::Exceptions::linear_solver_failed& e) {
      std::printf("max_iter = 2 rejected: %s\n", e.what());
    }
  } catch (const std::exception& e) {
    std::printf("failed: %s\n", e.what());
    rc = 5;
  }
  hdd_grid_destroy(g);
  if (rc == 0) std::printf("solve blocks ok\n");
  return rc;
}
