// many_check.cpp — the many-systems solve (CGMany.hpp, a thin layer over
// cgx_many_solve) from C++: a few 2-D Poisson systems on one pattern, system s
// with its values scaled by 1 + s / 4 and its own right-hand side, solved in
// one call and again one at a time by CG<double>::solve, and the solutions
// compared.
//
//   many_check [nx ny nsys]      (default 17 15 5; b_i = (i + 1) (s + 1))
// Both residuals are at most 1e-13 ||b||, so the solutions differ by at most
// 2 cond(A) 1e-13 relative; cond(A) < 120 at the default size (a scalar factor
// leaves it unchanged), hence the bar of 1e-10. Also counts the systems whose
// x and body count are identical to the single solve's (CG::solve runs its
// auto mode; the bit-for-bit pin to mode 1 is tests/test_gpu_many.py's).
// Prints one line and returns 0 when every system agrees, 1 otherwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "CG.hpp"
#include "CGMany.hpp"

using namespace CGSolver;

int main(int argc, char **argv) {
  const int nx = argc > 3 ? std::atoi(argv[1]) : 17, ny = argc > 3 ? std::atoi(argv[2]) : 15;
  const int nsys = argc > 3 ? std::atoi(argv[3]) : 5;
  if (nx < 1 || ny < 1 || nsys < 1) return 2;
  const int n = nx * ny;
  std::vector<int> rowptr(1, 0), col;
  std::vector<double> val;
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) {
      const int row = j * nx + i;
      if (j > 0) col.push_back(row - nx), val.push_back(-1.0);
      if (i > 0) col.push_back(row - 1), val.push_back(-1.0);
      col.push_back(row), val.push_back(4.0);
      if (i < nx - 1) col.push_back(row + 1), val.push_back(-1.0);
      if (j < ny - 1) col.push_back(row + nx), val.push_back(-1.0);
      rowptr.push_back((int)col.size());
    }
  const size_t nnz = val.size();
  std::vector<double> vals(nsys * nnz), B((size_t)nsys * n), X((size_t)nsys * n, 0.0);
  double nb = 0;
  for (int i = 0; i < n; ++i) nb += (i + 1.0) * (i + 1.0);
  for (int s = 0; s < nsys; ++s) {
    for (size_t e = 0; e < nnz; ++e) vals[s * nnz + e] = val[e] * (1.0 + 0.25 * s);
    for (int i = 0; i < n; ++i) B[(size_t)s * n + i] = (i + 1.0) * (s + 1.0);
  }

  acpp::sycl::queue q;
  CGMany<double> many(q, rowptr, col, vals);
  // one tolerance per call: 1e-13 of the smallest ||b||
  const double tol = 1e-13 * std::sqrt(nb);
  many.solve(B, X, tol);

  int bitwise = 0, agree = 0;
  double worst = 0;
  for (int s = 0; s < nsys; ++s) {
    std::vector<double> vs(vals.begin() + s * nnz, vals.begin() + (s + 1) * nnz);
    std::vector<double> bs(B.begin() + (size_t)s * n, B.begin() + (size_t)(s + 1) * n);
    std::vector<int> cs = col, rs = rowptr;
    CG<double> cg(q);
    cg.setMatrix(vs, cs, rs);
    cg.setTarget(bs);
    cg.solve(tol);
    const std::vector<double> xd = cg.extract();
    const double *xm = X.data() + (size_t)s * n;
    double num = 0, den = 0;
    for (int i = 0; i < n; ++i) {
      num += (xm[i] - xd[i]) * (xm[i] - xd[i]);
      den += xd[i] * xd[i];
    }
    const double rel = std::sqrt(num / den);
    if (rel > worst) worst = rel;
    if (rel <= 1e-10 && many.stopped()[s] == 1) ++agree;
    if (std::memcmp(xm, xd.data(), n * sizeof(double)) == 0 &&
        many.iterations()[s] == cg.iterations())
      ++bitwise;
  }
  const bool ok = agree == nsys;
  std::printf("many_check: %d systems of n = %d, %d agree with CG::solve to 1e-10 (worst relative "
              "difference %.3e), %d identical in x and bodies: %s\n",
              nsys, n, agree, worst, bitwise, ok ? "agreement" : "NO agreement");
  return ok ? 0 : 1;
}
