// examples/solve_main.cpp -- the whole hot path of the reference's driver on the device, through the C++ surface
// (include/hdd_discretizations.hh): SWIPDG::init() assembles ESV2007 on the 32 x 32 Q1 grid of [-1,1]^2, SWIPDG::solve
// does what ContainerBasedDefault::uncached_solve does (base.hh:327-367) -- theta-lincomb fused, apply_inverse by
// block-Jacobi preconditioned conjugate gradients (hdd_operator_solve).  Prints the iterations and the residual and
// exits non-zero unless the solve converged; a local solve on a BlockSWIPDG subdomain follows.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "hdd_discretizations.hh"

using namespace Dune::HDD::LinearElliptic;

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
    hdd_solve_info info{};
    const std::vector<double> u = sw.solve(0.0, Discretizations::SolverOptions(), &info);
    std::printf("solve kernels %s\n", hdd_last_solve_kernels());
    // the exact solution is cos(pi x / 2) cos(pi y / 2): its maximum is 1 at the origin
    double umax = 0.0;
    for (double v : u) umax = std::fmax(umax, v);
    std::printf("%s: %d iterations, residual %.3e, ||b|| %.3e, %zu dofs, max u %.4f\n",
                info.status == HDD_SOLVE_CONVERGED ? "converged" : "NOT converged", info.iterations, info.residual,
                info.rhs_norm, u.size(), umax);
    if (info.status != HDD_SOLVE_CONVERGED || !(info.residual <= 1e-8 * info.rhs_norm) || std::fabs(umax - 1.0) > 0.05) rc = 2;
    // max_iter too small: the reference's linear-solver exception
    Discretizations::SolverOptions few;
    few.max_iter = 2;
    try {
      sw.solve(0.0, few);
      std::printf("max_iter = 2 unexpectedly converged\n");
      rc = 3;
    } catch (const Dune::Stuff::Exceptions::linear_solver_failed& e) {
      std::printf("max_iter = 2 rejected: %s\n", e.what());
    }
  } catch (const std::exception& e) {
    std::printf("failed: %s\n", e.what());
    rc = 4;
  }
  hdd_grid_destroy(g);
  if (rc) return rc;

  // the local solve of subdomain 1 of a 2 x 2 BlockSWIPDG on the global arrays (block range, no extraction)
  hdd_structured_desc d2{HDD_SIMPLEX, 16, 16, 2, 2, HDD_BOUNDARY_ALL_DIRICHLET, 0, {-1.0, -1.0}, {1.0, 1.0}};
  if (hdd_grid_create_structured(&d2, &g) != HDD_OK) return 1;
  try {
    Problems::Problem esv;
    esv.force = Problems::ScalarFunction::cos_product(0.5 * M_PI * M_PI, 0.5 * M_PI, 0.5 * M_PI, 0.0, 3);
    Discretizations::BlockSWIPDG block(g, esv);
    block.init();
    const auto b = block.get_local_functional(1).affine_part();
    hdd_solve_info info{};
    const auto x = block.solve_local(1, b, 0.0, Discretizations::SolverOptions(), &info);
    // check it with the operator applied in place
    const auto y = block.apply_local_operator(1, x);
    double err = 0.0, nb = 0.0;
    for (size_t i = 0; i < b.size(); ++i) err += (y[i] - b[i]) * (y[i] - b[i]), nb += b[i] * b[i];
    std::printf("local solve: %d iterations, residual %.3e, true residual %.3e, ||b|| %.3e (%s)\n", info.iterations,
                info.residual, std::sqrt(err), std::sqrt(nb), hdd_last_solve_kernels());
    if (!(std::sqrt(err) <= 2e-8 * std::sqrt(nb))) rc = 5;
  } catch (const std::exception& e) {
    std::printf("failed: %s\n", e.what());
    rc = 6;
  }
  hdd_grid_destroy(g);
  if (rc == 0) std::printf("solve ok\n");
  return rc;
}
