// block_pcg_check.cpp — the block preconditioner extension of the drop-in
// CG.hpp (CGSolver::BlockPreconditioner, CG::setBlockPreconditioner) from
// C++: one matrix solved with block-Jacobi, then with the same blocks moved
// in as a Vector, then with Jacobi after the switch back. Inputs come from a
// raw file the test writes; outputs go to a raw file the test checks
// (tests/test_gpu_block_pcg.py).
//
//   block_pcg_check in.bin out.bin
// in.bin : int64 n, int64 nnz, int64 bs, int32 rowptr[n+1], int32 col[nnz],
//          f64 val[nnz], f64 b[n], f64 w[n * bs], f64 tol
// out.bin: per solve (block-Jacobi, Given, Jacobi): f64 iterations, f64 r.r
//          after the last body, f64 x[n]
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
  int64_t n = 0, nnz = 0, bs = 0;
  rd(f, &n, 1);
  rd(f, &nnz, 1);
  rd(f, &bs, 1);
  std::vector<int> rowptr(n + 1), col(nnz);
  std::vector<double> val(nnz), b(n), w(n * bs);
  double tol = 0;
  rd(f, rowptr.data(), rowptr.size());
  rd(f, col.data(), col.size());
  rd(f, val.data(), val.size());
  rd(f, b.data(), b.size());
  rd(f, w.data(), w.size());
  rd(f, &tol, 1);
  std::fclose(f);

  std::vector<double> out;
  auto solve = [&](CG<double> &cg) {
    std::vector<double> x0(n, 0.0);
    cg.setInital(x0);
    cg.solve(tol);
    out.push_back((double)cg.iterations());
    out.push_back(cg.finalResidualSquared());
    const std::vector<double> x = cg.extract();
    out.insert(out.end(), x.begin(), x.end());
  };
  acpp::sycl::queue q;
  CG<double> cg(q);
  cg.setMatrix(val, col, rowptr);
  cg.setTarget(b);
  cg.setBlockPreconditioner(BlockPreconditioner::Jacobi, (int)bs);
  if (cg.blockSize() != bs) return 3;
  solve(cg);
  cg.setBlockPreconditioner((int)bs, Vector<double>(q, w));  // moved in; implies Given
  if (cg.blockPreconditioner() != BlockPreconditioner::Given) return 3;
  solve(cg);
  cg.setPreconditioner(Preconditioner::Jacobi);  // replaces the block one
  if (cg.blockPreconditioner() != BlockPreconditioner::None) return 3;
  solve(cg);

  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  std::fwrite(out.data(), sizeof(double), out.size(), f);
  std::fclose(f);
  return 0;
}
