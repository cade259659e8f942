// examples/solve_multi_main.cpp -- the same affine components at several parameters in one device solve, through the
// C++ surface (include/hdd_discretizations.hh): OS2014, A(mu) = A_aff + mu A_1, on the 12 x 11 Kuhn grid, solved at
// four mu with one SWIPDG::solve(mus) (hdd_operator_solve_multi: the value arrays are read once per iteration for
// all four) and with four solve(mu).  Every column must be, byte for byte, what its single solve gives: the program
// prints a line per mu and exits non-zero otherwise.  Then two local right-hand sides at a mu each on one
// get_local_operator(ss) of a 2 x 2 BlockSWIPDG.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "hdd_discretizations.hh"

using namespace Dune::HDD::LinearElliptic;

namespace {
bool same_bytes(const std::vector<double>& a, const std::vector<double>& b)
{
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

bool same_info(const hdd_solve_info& a, const hdd_solve_info& b)
{
  return a.status == b.status && a.iterations == b.iterations && std::memcmp(&a.residual, &b.residual, sizeof(double)) == 0 &&
         std::memcmp(&a.rhs_norm, &b.rhs_norm, sizeof(double)) == 0;
}
}  // namespace

int main()
{
  const std::vector<double> mus{0.1, 0.3, 0.5, 1.0};   // A(mu) is positive definite on this grid for all four
  hdd_grid* g = nullptr;
  hdd_structured_desc d{HDD_SIMPLEX, 12, 11, 1, 1, HDD_BOUNDARY_ALL_DIRICHLET, 0, {-1.0, -1.0}, {1.0, 1.0}};
  if (hdd_grid_create_structured(&d, &g) != HDD_OK) return 1;
  int rc = 0;
  try {
    Discretizations::SWIPDG sw(g, Problems::OS2014());
    sw.init();
    std::vector<hdd_solve_info> infos;
    const auto X = sw.solve(mus, Discretizations::SolverOptions(), &infos);
    std::printf("solve kernels %s\n", hdd_last_solve_kernels());
    if (std::string(hdd_last_solve_kernels()).find("apply_tile_multi_kernel<3, 3, 4, dot> + cg_update<3, 4, own>") == std::string::npos) rc = 2;
    for (size_t j = 0; j < mus.size(); ++j) {
      hdd_solve_info one{};
      const auto x = sw.solve(mus[j], Discretizations::SolverOptions(), &one);
      const bool same = same_bytes(x, X[j]) && same_info(one, infos[j]);
      std::printf("%s: mu %.2f, %d iterations, residual %.3e, ||b|| %.3e, %s the single solve\n",
                  infos[j].status == HDD_SOLVE_CONVERGED ? "converged" : "NOT converged", mus[j], infos[j].iterations,
                  infos[j].residual, infos[j].rhs_norm, same ? "bit-identical to" : "DIFFERS from");
      if (infos[j].status != HDD_SOLVE_CONVERGED || !(infos[j].residual <= 1e-8 * infos[j].rhs_norm) || !same) rc = 3;
    }
    // max_iter too small: the reference's linear-solver exception names the first column that failed and its mu
    Discretizations::SolverOptions few;
    few.max_iter = 2;
    try {
      sw.solve(mus, few);
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
  if (rc) return rc;

  // two local right-hand sides on subdomain 1 of a 2 x 2 BlockSWIPDG, each at its own mu (a principal block of a
  // positive definite matrix: 16 x 16 is definite for mu >= 0.5)
  hdd_structured_desc d2{HDD_SIMPLEX, 16, 16, 2, 2, HDD_BOUNDARY_ALL_DIRICHLET, 0, {-1.0, -1.0}, {1.0, 1.0}};
  if (hdd_grid_create_structured(&d2, &g) != HDD_OK) return 1;
  try {
    Discretizations::BlockSWIPDG block(g, Problems::OS2014());
    block.init();
    const std::vector<double> local_mus{0.6, 1.0};
    const std::vector<std::vector<double>> B(2, block.get_local_functional(1).affine_part());
    std::vector<hdd_solve_info> infos;
    const auto X = block.solve_local(1, B, local_mus, Discretizations::SolverOptions(), &infos);
    for (size_t j = 0; j < B.size(); ++j) {
      hdd_solve_info one{};
      const auto x = block.solve_local(1, B[j], local_mus[j], Discretizations::SolverOptions(), &one);
      const bool same = same_bytes(x, X[j]) && same_info(one, infos[j]);
      std::printf("%s: local mu %.2f, %d iterations, residual %.3e, ||b|| %.3e, %s the single solve\n",
                  infos[j].status == HDD_SOLVE_CONVERGED ? "converged" : "NOT converged", local_mus[j], infos[j].iterations,
                  infos[j].residual, infos[j].rhs_norm, same ? "bit-identical to" : "DIFFERS from");
      if (infos[j].status != HDD_SOLVE_CONVERGED || !same) rc = 6;
    }
  } catch (const std::exception& e) {
    std::printf("failed: %s\n", e.what());
    rc = 7;
  }
  hdd_grid_destroy(g);
  if (rc == 0) std::printf("solve multi ok\n");
  return rc;
}
