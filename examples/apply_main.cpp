// examples/apply_main.cpp -- applying the assembled operators on the device through the C++ surface
// (include/hdd_discretizations.hh), the way the reference's consumers use them: pyMOR's apply / apply2 on the
// affinely decomposed system matrix at a parameter (base.hh:45, 260-264) and LRBMS's local / coupling operators
// (block-swipdg.hh:625-676) -- here without freeze_parameter's A(mu) and without extracting a block.
// Writes its inputs and outputs as raw arrays to <outdir> for tests/test_gpu_apply_surface.py to compare with the
// CPU oracle's matrices times the same vectors.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "hdd_discretizations.hh"

using namespace Dune::HDD::LinearElliptic;

template <class T>
static void dump(const std::string& path, const std::vector<T>& v)
{
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), std::streamsize(v.size() * sizeof(T)));
}

// a reproducible vector with entries in (-1, 1) (64-bit LCG)
static std::vector<double> vec(size_t n, uint64_t seed)
{
  std::vector<double> v(n);
  uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
  for (auto& x : v) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    x = double(int64_t(s >> 11) - (int64_t(1) << 52)) / double(int64_t(1) << 52);
  }
  return v;
}

int main(int argc, char** argv)
{
  const std::string out = argc > 1 ? argv[1] : ".";
  // 1. ESV2007 on the 16 x 16 Kuhn grid of [-1,1]^2 in 2 x 2 subdomains: the global operator and its blocks
  hdd_structured_desc d{HDD_SIMPLEX, 16, 16, 2, 2, HDD_BOUNDARY_ALL_DIRICHLET, 0, {-1.0, -1.0}, {1.0, 1.0}};
  hdd_grid* g = nullptr;
  if (hdd_grid_create_structured(&d, &g) != HDD_OK) return 1;
  {
    Problems::Problem esv;   // kappa = 1 (affine part), A = I
    esv.force = Problems::ScalarFunction::cos_product(0.5 * M_PI * M_PI, 0.5 * M_PI, 0.5 * M_PI, 0.0, 3);
    Discretizations::BlockSWIPDG block(g, esv);
    block.init();
    const auto& A = block.system_matrix();
    const auto x = vec(size_t(block.num_dofs()), 1), v = vec(size_t(block.num_dofs()), 2);
    dump(out + "/block_x.bin", x);
    dump(out + "/block_v.bin", v);
    dump(out + "/block_y.bin", A.apply(x));
    std::printf("block apply kernel %s\n", hdd_last_apply_kernel());
    dump(out + "/block_vAx.bin", std::vector<double>{A.apply2(v, x)});
    const auto nbs = block.neighbouring_subdomains(0);
    const int nn = nbs.at(0);
    dump(out + "/neighbour0.bin", std::vector<int32_t>{nn});
    const auto x0 = block.localize_vector(x, 0), xn = block.localize_vector(x, nn);
    dump(out + "/local0_y.bin", block.apply_local_operator(0, x0));
    std::printf("local apply kernel %s\n", hdd_last_apply_kernel());
    dump(out + "/coupling0_y.bin", block.apply_coupling_operator(0, nn, xn));
    // the extracted operators give the same vectors through the CSR kernel
    const auto yl = block.get_local_operator(0).apply(x0);
    std::printf("extracted apply kernel %s\n", hdd_last_apply_kernel());
    dump(out + "/local0_y_extracted.bin", yl);
    dump(out + "/coupling0_y_extracted.bin", block.get_coupling_operator(0, nn).apply(xn));
    try {
      block.apply_coupling_operator(0, 3, block.localize_vector(x, 3));   // diagonal subdomain: not a face neighbour
      std::printf("coupling(0,3) unexpectedly applied\n");
    } catch (const std::out_of_range& e) {
      std::printf("coupling(0,3) rejected: %s\n", e.what());
    }
    try {
      A.apply(std::vector<double>(3, 1.0));
      std::printf("short vector unexpectedly accepted\n");
    } catch (const std::invalid_argument& e) {
      std::printf("short vector rejected: %s\n", e.what());
    }
  }
  hdd_grid_destroy(g);

  // 2. OS2014 on 8 x 8 Kuhn: A(mu) = A_aff + mu A_1 applied at mu = 0 and mu = 0.3 without writing A(mu)
  hdd_structured_desc d2{HDD_SIMPLEX, 8, 8, 1, 1, HDD_BOUNDARY_ALL_DIRICHLET, 0, {-1.0, -1.0}, {1.0, 1.0}};
  if (hdd_grid_create_structured(&d2, &g) != HDD_OK) return 1;
  {
    Problems::Problem os;
    const double kx = 4.0 * M_PI, ky = 2.0 * M_PI;
    os.diffusion_factor.affine_part = Problems::ScalarFunction::sinusoid(1.0, 0.75, kx, ky, 3);
    os.diffusion_factor.components.push_back(Problems::ScalarFunction::sinusoid(0.0, -0.75, kx, ky, 3));
    os.diffusion_factor.coefficients.emplace_back("mu", "mu", 1.0);
    Discretizations::SWIPDG sw(g, os);
    sw.init();
    const auto& A = sw.system_matrix();
    const auto x = vec(size_t(sw.num_dofs()), 3), v = vec(size_t(sw.num_dofs()), 4);
    dump(out + "/os_x.bin", x);
    dump(out + "/os_v.bin", v);
    dump(out + "/os_y_0.bin", A.apply(x));
    dump(out + "/os_y_0.3.bin", A.apply(x, 0.3));
    std::printf("os2014 apply kernel %s\n", hdd_last_apply_kernel());
    dump(out + "/os_vAx_0.3.bin", std::vector<double>{A.apply2(v, x, 0.3)});
  }
  hdd_grid_destroy(g);
  std::printf("apply ok\n");
  return 0;
}
