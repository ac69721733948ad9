// shift_check.cpp — the multi-shift solve of the drop-in CG.hpp
// (CG::solveShifted, an extension over cgx_cg_solve_shifted) from C++: one
// matrix and right-hand side under k diagonal shifts, each shift's result
// written out for the test to compare with the C ABI's
// (tests/test_gpu_shift.py).
//
//   shift_check in.bin out.bin
// in.bin : int64 n, int64 nnz, int64 k, int64 max_iter, int32 rowptr[n+1],
//          int32 col[nnz], f64 val[nnz], f64 b[n], f64 sigma[k], f64 tol
// out.bin: per shift: f64 iterations, f64 |zeta| ||r|| after the last body,
//          f64 stop code, f64 x[n]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "CG.hpp"

using namespace CGSolver;

template <class T> static void rd(FILE *f, T *p, size_t n) {
  if (std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "short read\n");
    std::exit(2);
  }
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t n = 0, nnz = 0, k = 0, max_iter = -1;
  rd(f, &n, 1);
  rd(f, &nnz, 1);
  rd(f, &k, 1);
  rd(f, &max_iter, 1);
  std::vector<int> rowptr(n + 1), col(nnz);
  std::vector<double> val(nnz), b(n), sigma(k);
  double tol = 0;
  rd(f, rowptr.data(), rowptr.size());
  rd(f, col.data(), col.size());
  rd(f, val.data(), val.size());
  rd(f, b.data(), b.size());
  rd(f, sigma.data(), sigma.size());
  rd(f, &tol, 1);
  std::fclose(f);

  acpp::sycl::queue q;
  CG<double> cg(q);
  cg.setMatrix(val, col, rowptr);
  cg.setTarget(b);
  cg.setMaxIterations(max_iter);
  std::vector<Vector<double>> X;
  cg.solveShifted(sigma, X, tol);

  std::vector<double> out;
  for (int64_t c = 0; c < k; ++c) {
    out.push_back((double)cg.shiftedIterations()[c]);
    out.push_back(cg.shiftedResidual()[c]);
    out.push_back((double)cg.shiftedStopped()[c]);
    std::vector<double> x(n);
    if (cgx_d2h(q.native(), x.data(), X[c].ptr(), n * sizeof(double)) != 0) return 3;
    out.insert(out.end(), x.begin(), x.end());
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(out.data(), sizeof(double), out.size(), f);
  std::fclose(f);
  return 0;
}
