// examples/project_main.cpp -- the reduced-basis step through the C++ surface (include/hdd_discretizations.hh): OS2014,
// A(mu) = A_aff + mu A_1, on the 12 x 11 Kuhn grid.  Snapshots at three mu with one SWIPDG::solve(mus), a host
// Gram-Schmidt, then SWIPDG::project(basis): every operator term G_q = V^T A_q V in one pass over the value arrays
// (hdd_operator_project), the right-hand side terms through hdd_vectors_inner.  Every entry of every G_q is compared
// with the route there was before -- one hdd_operator_apply2 call per term -- and with the same sums on the host:
//   |G - G_host|_ij <= B_ij := 2 gamma_K (|V|^T |A_q| |V|)_ij,  K = rows + longest row + 3  (any order of summation),
//   |G - G_apply2|_ij <= 2 B_ij                                  (both lie within B of the exact value);
// the program exits non-zero otherwise.  Then the reduced problem is solved at the first mu and the distance of the
// reconstruction to that snapshot is printed (for information: it depends on the solver tolerance and the
// conditioning).  Last, the reduced local and coupling operators of a 2 x 2 BlockSWIPDG through a block range,
// against the host sums on the same rows and columns.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "hdd_discretizations.hh"

using namespace Dune::HDD::LinearElliptic;
using Vectors = std::vector<std::vector<double>>;

namespace {
double gamma_of(double n) { return n * 0x1p-53 / (1.0 - n * 0x1p-53); }

// V^T A U and the bound B of the header on rows [r0, r1), columns [c0, c1) of the host arrays; row-major [n_v][n_u]
void host_sums(const std::vector<int64_t>& rp, const std::vector<int32_t>& col, const std::vector<double>& vals, int64_t r0, int64_t r1,
               int64_t c0, int64_t c1, const Vectors& V, const Vectors& U, std::vector<double>& ref, std::vector<double>& bound)
{
  const size_t nv = V.size(), nu = U.size();
  ref.assign(nv * nu, 0.0);
  bound.assign(nv * nu, 0.0);
  int64_t longest = 0;
  std::vector<double> w(nu), aw(nu);
  for (int64_t r = r0; r < r1; ++r) {
    std::fill(w.begin(), w.end(), 0.0);
    std::fill(aw.begin(), aw.end(), 0.0);
    int64_t len = 0;
    for (int64_t k = rp[size_t(r)]; k < rp[size_t(r) + 1]; ++k) {
      const int64_t c = col[size_t(k)];
      if (c < c0 || c >= c1) continue;
      ++len;
      for (size_t j = 0; j < nu; ++j) {
        w[j] += vals[size_t(k)] * U[j][size_t(c - c0)];
        aw[j] += std::fabs(vals[size_t(k)] * U[j][size_t(c - c0)]);
      }
    }
    longest = std::max(longest, len);
    for (size_t i = 0; i < nv; ++i)
      for (size_t j = 0; j < nu; ++j) {
        ref[i * nu + j] += V[i][size_t(r - r0)] * w[j];
        bound[i * nu + j] += std::fabs(V[i][size_t(r - r0)]) * aw[j];
      }
  }
  const double g = 2.0 * gamma_of(double(r1 - r0 + longest + 3));
  for (double& b : bound) b *= g;
}

// the largest |got - want| / (factor * bound) over the entries (0 / 0 counts as 0, x / 0 as infinity)
double worst(const std::vector<double>& got, const std::vector<double>& want, const std::vector<double>& bound, double factor)
{
  double m = 0.0;
  for (size_t k = 0; k < got.size(); ++k) {
    const double e = std::fabs(got[k] - want[k]);
    if (!(e <= factor * bound[k])) m = std::max(m, bound[k] > 0.0 ? e / (factor * bound[k]) : HUGE_VAL);
    else if (bound[k] > 0.0) m = std::max(m, e / (factor * bound[k]));
  }
  return m;
}

// modified Gram-Schmidt in the Euclidean product, twice
Vectors orthonormalize(Vectors X)
{
  for (size_t i = 0; i < X.size(); ++i) {
    for (int pass = 0; pass < 2; ++pass)
      for (size_t k = 0; k < i; ++k) {
        double s = 0.0;
        for (size_t r = 0; r < X[i].size(); ++r) s += X[k][r] * X[i][r];
        for (size_t r = 0; r < X[i].size(); ++r) X[i][r] -= s * X[k][r];
      }
    double n = 0.0;
    for (const double x : X[i]) n += x * x;
    n = std::sqrt(n);
    if (!(n > 0.0)) throw std::runtime_error("orthonormalize: linearly dependent snapshots");
    for (double& x : X[i]) x /= n;
  }
  return X;
}

// the terms of A(mu) in project()'s order: the affine part first, then the components
std::vector<const internal::DeviceArray<double>*> terms_of(const Discretizations::AffinelyDecomposedMatrix& A)
{
  std::vector<const internal::DeviceArray<double>*> t;
  if (A.affine) t.push_back(A.affine.get());
  for (const auto& c : A.comps) t.push_back(c.get());
  return t;
}

std::vector<double> host_values(const internal::DeviceArray<double>& a, int64_t nnz)
{
  auto h = a.download();
  h.resize(size_t(nnz));
  return h;
}
}  // namespace

int main()
{
  const std::vector<double> mus{0.1, 0.5, 1.0};   // A(mu) is positive definite on this grid for all three
  hdd_grid* g = nullptr;
  hdd_structured_desc d{HDD_SIMPLEX, 12, 11, 1, 1, HDD_BOUNDARY_ALL_DIRICHLET, 0, {-1.0, -1.0}, {1.0, 1.0}};
  if (hdd_grid_create_structured(&d, &g) != HDD_OK) return 1;
  int rc = 0;
  try {
    Discretizations::SWIPDG sw(g, Problems::OS2014());
    sw.init();
    const auto X = sw.solve(mus);
    const Vectors basis = orthonormalize(X);
    const auto R = sw.project(basis);
    std::printf("project kernel %s\n", hdd_last_apply_kernel());
    const auto& A = sw.system_matrix();
    const auto terms = terms_of(A);
    if (R.operators.size() != terms.size() || R.n != int(basis.size())) rc = 2;
    if (std::string(hdd_last_apply_kernel()) != "project_tile_kernel<3, 3>") rc = 2;
    // the route there was before: hdd_operator_apply2 per term (one chunk: three vectors a side)
    const int64_t rows = A.pattern->rows, ld = rows;
    const int32_t n = int32_t(basis.size());
    std::vector<double> flat;
    for (const auto& b : basis) flat.insert(flat.end(), b.begin(), b.end());
    internal::DeviceArray<double> dv(flat), work{size_t(n) * size_t(ld)}, out{size_t(n) * size_t(n)};
    const hdd_csr pat = A.pattern->csr();
    for (size_t q = 0; q < terms.size() && rc == 0; ++q) {
      const double* vals = terms[q]->get();
      internal::check(hdd_operator_apply2(A.ctx, A.tile_nbrs ? &A.tile_mesh : nullptr, &pat, &vals, 1, nullptr, nullptr, dv.get(), ld, n,
                                          dv.get(), ld, n, work.get(), ld, out.get(), nullptr),
                      "hdd_operator_apply2");
      internal::hip_check(hipDeviceSynchronize(), "apply2");
      auto old = out.download();
      old.resize(size_t(n) * size_t(n));
      std::vector<double> ref, bound;
      host_sums(A.pattern->row_ptr(), A.pattern->col(), host_values(*terms[q], A.pattern->nnz), 0, rows, 0, A.pattern->cols, basis, basis,
                ref, bound);
      const double w_host = worst(R.operators[q], ref, bound, 1.0), w_old = worst(R.operators[q], old, bound, 2.0);
      std::printf("term %zu: G[0][0] %.15e, error / bound %.3f against the host sums, %.3f against apply2\n", q, R.operators[q][0], w_host,
                  w_old);
      if (!(w_host <= 1.0) || !(w_old <= 1.0)) rc = 3;
    }
    // the reduced solve at the first mu against its snapshot
    const auto c = R.solve(mus[0]);
    double diff = 0.0, norm = 0.0;
    for (size_t r = 0; r < X[0].size(); ++r) {
      double u = 0.0;
      for (size_t i = 0; i < basis.size(); ++i) u += c[i] * basis[i][r];
      diff += (u - X[0][r]) * (u - X[0][r]);
      norm += X[0][r] * X[0][r];
    }
    std::printf("reproduction error at mu %.2f: %.3e\n", mus[0], std::sqrt(diff / norm));
  } catch (const std::exception& e) {
    std::printf("failed: %s\n", e.what());
    rc = 5;
  }
  hdd_grid_destroy(g);
  if (rc) return rc;

  // reduced local and coupling operators of subdomain 1 of a 2 x 2 BlockSWIPDG: the blocks in place, no extraction
  hdd_structured_desc d2{HDD_SIMPLEX, 16, 16, 2, 2, HDD_BOUNDARY_ALL_DIRICHLET, 0, {-1.0, -1.0}, {1.0, 1.0}};
  if (hdd_grid_create_structured(&d2, &g) != HDD_OK) return 1;
  try {
    Discretizations::BlockSWIPDG block(g, Problems::OS2014());
    block.init();
    const int ss = 1, nn = block.neighbouring_subdomains(ss).at(0);
    const auto& A = block.system_matrix();
    const auto terms = terms_of(A);
    const int64_t nb = 3;
    int64_t a, b, p, q;
    internal::check(hdd_grid_subdomain_range(g, ss, ss + 1, &a, &b), "range");
    internal::check(hdd_grid_subdomain_range(g, nn, nn + 1, &p, &q), "range");
    auto wave = [](int64_t size, double k) {
      std::vector<double> v(static_cast<size_t>(size));
      for (size_t r = 0; r < v.size(); ++r) v[r] = std::cos(k * double(r + 1));
      return v;
    };
    const Vectors Vs{wave((b - a) * nb, 0.37), wave((b - a) * nb, 1.1)}, Vn{wave((q - p) * nb, 0.73), wave((q - p) * nb, 0.21), wave((q - p) * nb, 2.3)};
    const auto L = block.project_local(ss, Vs), C = block.project_coupling(ss, nn, Vs, Vn);
    for (size_t t = 0; t < terms.size(); ++t) {
      const auto vals = host_values(*terms[t], A.pattern->nnz);
      std::vector<double> ref, bound;
      host_sums(A.pattern->row_ptr(), A.pattern->col(), vals, a * nb, b * nb, a * nb, b * nb, Vs, Vs, ref, bound);
      const double wl = worst(L.at(t), ref, bound, 1.0);
      host_sums(A.pattern->row_ptr(), A.pattern->col(), vals, a * nb, b * nb, p * nb, q * nb, Vs, Vn, ref, bound);
      const double wc = worst(C.at(t), ref, bound, 1.0);
      std::printf("term %zu: local (%d, %d) error / bound %.3f, coupling (%d, %d) error / bound %.3f\n", t, ss, ss, wl, ss, nn, wc);
      if (!(wl <= 1.0) || !(wc <= 1.0)) rc = 6;
    }
  } catch (const std::exception& e) {
    std::printf("failed: %s\n", e.what());
    rc = 7;
  }
  hdd_grid_destroy(g);
  if (rc == 0) std::printf("project ok\n");
  return rc;
}
