// examples/solve_batched_main.cpp -- several right-hand sides against one matrix in one device solve, through the C++
// surface (include/hdd_discretizations.hh): SWIPDG::solve on three right-hand sides of ESV2007 on the 32 x 32 Q1 grid
// (hdd_operator_solve_batched: pyMOR's apply_inverse on a VectorArray), then two local right-hand sides on one
// get_local_operator(ss) of a 2 x 2 BlockSWIPDG.  Every column must be, byte for byte, what the single solve gives
// for it: the program exits non-zero otherwise.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "hdd_discretizations.hh"

using namespace Dune::HDD::LinearElliptic;

namespace {
// the right-hand side the discretization assembled, and variations of it with other spectra
std::vector<std::vector<double>> columns(const std::vector<double>& b, int n)
{
  std::vector<std::vector<double>> B(size_t(n), b);
  for (int j = 1; j < n; ++j)
    for (size_t i = 0; i < b.size(); ++i) B[size_t(j)][i] = b[i] * std::cos(0.37 * j * double(i)) + 1e-3 * std::sin(0.11 * j * double(i));
  return B;
}

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
  hdd_grid* g = nullptr;
  hdd_structured_desc d{HDD_CUBE, 32, 32, 1, 1, HDD_BOUNDARY_ALL_DIRICHLET, 0, {-1.0, -1.0}, {1.0, 1.0}};
  if (hdd_grid_create_structured(&d, &g) != HDD_OK) return 1;
  int rc = 0;
  try {
    Problems::Problem esv;   // kappa = 1 (affine part), A = I
    esv.force = Problems::ScalarFunction::cos_product(0.5 * M_PI * M_PI, 0.5 * M_PI, 0.5 * M_PI, 0.0, 3);
    Discretizations::SWIPDG sw(g, esv);
    sw.init();
    const auto B = columns(sw.rhs().affine_part(), 3);
    std::vector<hdd_solve_info> infos;
    const auto X = sw.solve(B, 0.0, Discretizations::SolverOptions(), &infos);
    std::printf("solve kernels %s\n", hdd_last_solve_kernels());
    if (std::string(hdd_last_solve_kernels()).find("cg_direction<4>") == std::string::npos) rc = 2;
    for (size_t j = 0; j < B.size(); ++j) {
      hdd_solve_info one{};
      const auto x = sw.system_matrix().apply_inverse(B[j], 0.0, Discretizations::SolverOptions(), nullptr, &one);
      const bool same = same_bytes(x, X[j]) && same_info(one, infos[j]);
      std::printf("%s: column %zu, %d iterations, residual %.3e, ||b|| %.3e, %s the single solve\n",
                  infos[j].status == HDD_SOLVE_CONVERGED ? "converged" : "NOT converged", j, infos[j].iterations,
                  infos[j].residual, infos[j].rhs_norm, same ? "bit-identical to" : "DIFFERS from");
      if (infos[j].status != HDD_SOLVE_CONVERGED || !(infos[j].residual <= 1e-8 * infos[j].rhs_norm) || !same) rc = 3;
    }
    // max_iter too small: the reference's linear-solver exception names the first column that failed
    Discretizations::SolverOptions few;
    few.max_iter = 2;
    try {
      sw.solve(B, 0.0, few);
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

  // two local right-hand sides on subdomain 1 of a 2 x 2 BlockSWIPDG (block range on the global arrays)
  hdd_structured_desc d2{HDD_SIMPLEX, 16, 16, 2, 2, HDD_BOUNDARY_ALL_DIRICHLET, 0, {-1.0, -1.0}, {1.0, 1.0}};
  if (hdd_grid_create_structured(&d2, &g) != HDD_OK) return 1;
  try {
    Problems::Problem esv;
    esv.force = Problems::ScalarFunction::cos_product(0.5 * M_PI * M_PI, 0.5 * M_PI, 0.5 * M_PI, 0.0, 3);
    Discretizations::BlockSWIPDG block(g, esv);
    block.init();
    const auto B = columns(block.get_local_functional(1).affine_part(), 2);
    std::vector<hdd_solve_info> infos;
    const auto X = block.solve_local(1, B, 0.0, Discretizations::SolverOptions(), &infos);
    for (size_t j = 0; j < B.size(); ++j) {
      hdd_solve_info one{};
      const auto x = block.solve_local(1, B[j], 0.0, Discretizations::SolverOptions(), &one);
      const bool same = same_bytes(x, X[j]) && same_info(one, infos[j]);
      std::printf("%s: local column %zu, %d iterations, residual %.3e, ||b|| %.3e, %s the single solve\n",
                  infos[j].status == HDD_SOLVE_CONVERGED ? "converged" : "NOT converged", j, infos[j].iterations,
                  infos[j].residual, infos[j].rhs_norm, same ? "bit-identical to" : "DIFFERS from");
      if (infos[j].status != HDD_SOLVE_CONVERGED || !same) rc = 6;
    }
  } catch (const std::exception& e) {
    std::printf("failed: %s\n", e.what());
    rc = 7;
  }
  hdd_grid_destroy(g);
  if (rc == 0) std::printf("solve batched ok\n");
  return rc;
}
