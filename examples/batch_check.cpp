// batch_check.cpp — the batched solve of the drop-in CG.hpp (CG::solveBatch,
// an extension over cgx_cg_solve_batch) from C++: k right-hand sides on one
// matrix, each column's result written out for the test to compare with the
// single solves (tests/test_gpu_batch.py).
//
//   batch_check in.bin out.bin [form]
// in.bin : int64 n, int64 nnz, int64 k, int64 max_iter, int32 rowptr[n+1],
//          int32 col[nnz], f64 val[nnz], f64 B[k][n], f64 tol
// out.bin: per column: f64 iterations, f64 r.r after the last body, f64 stop
//          code, f64 x[n]
// form   : 0 auto (default), 1 fused, 2 sequential
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
  std::vector<double> val(nnz);
  std::vector<std::vector<double>> b(k, std::vector<double>(n));
  double tol = 0;
  rd(f, rowptr.data(), rowptr.size());
  rd(f, col.data(), col.size());
  rd(f, val.data(), val.size());
  for (auto &bc : b) rd(f, bc.data(), bc.size());
  rd(f, &tol, 1);
  std::fclose(f);

  acpp::sycl::queue q;
  CG<double> cg(q);
  cg.setMatrix(val, col, rowptr);
  cg.setMaxIterations(max_iter);
  cg.setBatchForm(argc > 3 ? std::atoi(argv[3]) : 0);
  std::vector<Vector<double>> B, X;
  for (auto &bc : b) {
    B.emplace_back(q, bc);
    X.emplace_back(q);  // unallocated: a zero initial guess
  }
  cg.solveBatch(B, X, tol);

  std::vector<double> out;
  for (int64_t c = 0; c < k; ++c) {
    out.push_back((double)cg.batchIterations()[c]);
    out.push_back(cg.batchFinalResidualSquared()[c]);
    out.push_back((double)cg.batchStopped()[c]);
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
