// dune-hdd_amd/csrc/host/quadrature.hh -- host quadrature rules and 1D Lagrange tables (internal).
// Pure host arithmetic: every matrix and functional the library assembles is integrated with these, so they are
// plain C++ that the CPU suite and the host sanitizer program reach directly.  The library compiles quadrature.cpp
// with the device code's floating-point flags (Makefile FPFLAGS): the tables then match, bit for bit, those of the
// time when these functions were the host half of a kernel file.
#pragma once

#pragma GCC visibility push(hidden)   // internal: not part of the library's exported symbols
namespace hdd {

// n-point Gauss-Legendre rule on [0, 1] (Newton on P_n), points ascending; n >= 1
void gauss_legendre01(int n, double* x, double* w);

// equidistant Lagrange polynomial k of degree p and its derivative at x
void lagrange_1d(int p, int k, double x, double* v, double* d);

// Rules as rows {point (3, unused coordinates 0), weight}; return the number of points, or -1 if it exceeds cap.
// simplex_rule: reference triangle (area 1/2), exact for the given order.  tensor_rule: (order + 2) / 2
// Gauss-Legendre points per direction on [0, 1]^dim.
int simplex_rule(int order, double (*q)[4], int cap);
int tensor_rule(int dim, int order, double (*q)[4], int cap);
// tensor_rule of a face (fdim <= 2) as rows {face parameters (2), weight}
int face_rule(int fdim, int order, double (*q)[3], int cap);

// The 1D reference tables of Q_p on hexahedra, in the layout of hdd::dev::HexTables (swipdg_kernels.hh, which
// includes HIP and so cannot be named here): Gauss-Legendre points / weights of the volume (nq1v) and face (nq1f)
// rules, the degree-p Lagrange polynomials and derivatives at those points and at 0 and 1.
struct HexTableRefs {
  double *sv, *wv, *sf, *wf;
  double (*Lv)[8], (*Dv)[8], (*Lf)[8], (*Df)[8];
  double (*Le)[2], (*De)[2];
};
void hex_tables(int degree, int nq1v, int nq1f, const HexTableRefs& t);

}  // namespace hdd
#pragma GCC visibility pop
