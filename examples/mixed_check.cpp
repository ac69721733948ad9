// mixed_check.cpp — the mixed-precision solve of the drop-in CG.hpp
// (CG<double>::solveMixed, an extension over cgx_mixed_solve) from C++: a 2-D
// Poisson system solved to 1e-13 ||b|| by f32 bodies inside f64 refinement and
// again by the plain f64 solve, and the two solutions compared.
//
//   mixed_check [nx ny]          (default 17 15; b_i = i + 1)
// Both residuals are at most 1e-13 ||b||, so the solutions differ by at most
// 2 cond(A) 1e-13 relative; cond(A) < 120 at the default size, hence the bar
// of 1e-10. Prints one line and returns 0 when they agree, 1 otherwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "CG.hpp"

using namespace CGSolver;

int main(int argc, char **argv) {
  const int nx = argc > 2 ? std::atoi(argv[1]) : 17, ny = argc > 2 ? std::atoi(argv[2]) : 15;
  if (nx < 1 || ny < 1) return 2;
  const int n = nx * ny;
  std::vector<int> rowptr(1, 0), col;
  std::vector<double> val, b(n);
  for (int j = 0; j < ny; ++j)
    for (int i = 0; i < nx; ++i) {
      const int row = j * nx + i;
      if (j > 0) col.push_back(row - nx), val.push_back(-1.0);
      if (i > 0) col.push_back(row - 1), val.push_back(-1.0);
      col.push_back(row), val.push_back(4.0);
      if (i < nx - 1) col.push_back(row + 1), val.push_back(-1.0);
      if (j < ny - 1) col.push_back(row + nx), val.push_back(-1.0);
      rowptr.push_back((int)col.size());
      b[row] = row + 1.0;
    }
  double nb = 0;
  for (double v : b) nb += v * v;
  const double tol = 1e-13 * std::sqrt(nb);

  acpp::sycl::queue q;
  CG<double> cg(q);
  cg.setMatrix(val, col, rowptr);
  cg.setTarget(b);
  cg.solveMixed(tol);
  const std::vector<double> xm = cg.extract();
  const int status = cg.mixedStatus(), outer = cg.outerSteps();
  const long long inner = cg.iterations();
  long long bytes = 0;
  {
    int64_t by = 0;
    if (cgx_mixed_bytes(cg.mixedHandle(), &by) != 0) return 3;
    bytes = by;
  }

  std::vector<double> zero(n, 0.0);
  cg.setInital(zero);
  cg.solve(tol);
  const std::vector<double> xd = cg.extract();
  double num = 0, den = 0;
  for (int i = 0; i < n; ++i) {
    num += (xm[i] - xd[i]) * (xm[i] - xd[i]);
    den += xd[i] * xd[i];
  }
  const double rel = std::sqrt(num / den);
  const bool ok = rel <= 1e-10;
  std::printf("mixed_check: n = %d, mixed status %d after %d outer steps and %lld bodies, f64 "
              "solve %lld bodies, %lld device bytes added, relative difference %.3e: %s\n",
              n, status, outer, inner, cg.iterations(), bytes, rel,
              ok ? "agreement to 1e-10" : "NO agreement to 1e-10");
  return ok ? 0 : 1;
}
