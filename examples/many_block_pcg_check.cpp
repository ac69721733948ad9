// many_block_pcg_check.cpp — block-Jacobi preconditioning of the many-systems
// solve (CGMany::setBlockPreconditioner, a thin layer over
// cgx_many_set_block_precond) from C++: a few vector-valued systems on one
// pattern, A = D^T (L (x) I_3) D with L the 5-point Laplacian on nx x ny nodes,
// 3 unknowns per node and D = blockdiag(T_k), T_k = diag(1, 6, 30) Q_k with Q_k
// a rotation that changes from node to node: the conditioning sits inside each
// node's dense 3 x 3 block, where a diagonal preconditioner does little and
// block-Jacobi undoes it. System s is scaled symmetrically, d_i = 10^(s ((7 i)
// mod 11) / (44 nsys)).
//
//   many_block_pcg_check [nx ny nsys]      (default 6 5 4; b_i = 1 + (i mod 7))
// Solves the set with Jacobi, with CGX_BLOCK_JACOBI (bs = 3) and with
// CGX_BLOCK_GIVEN on the array blockInverse(3) returns, and checks, printing
// one line and returning 0 when all hold, 1 otherwise:
//  - JACOBI and GIVEN agree bit for bit in x, bodies, r.r and r.z (the same W,
//    formed by the solve or read from the caller's array);
//  - every system stops by the rule under both block solves (Jacobi may end
//    at its cap of n + 1 bodies: at the default size it does);
//  - block-Jacobi needs fewer bodies than Jacobi, summed over the systems.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "CGMany.hpp"

using namespace CGSolver;

int main(int argc, char **argv) {
  const int nx = argc > 3 ? std::atoi(argv[1]) : 6, ny = argc > 3 ? std::atoi(argv[2]) : 5;
  const int nsys = argc > 3 ? std::atoi(argv[3]) : 4;
  if (nx < 1 || ny < 1 || nsys < 1) return 2;
  const int bs = 3, nn = nx * ny, n = nn * bs;
  // T_k = diag(1, 6, 30) Q_k, Q_k = Rz(a_k) Rx(c_k)
  std::vector<double> T((size_t)nn * 9);
  for (int k = 0; k < nn; ++k) {
    const double a = 0.7 + 1.3 * k, c = 0.4 + 0.9 * ((5 * k) % 7);
    const double ca = std::cos(a), sa = std::sin(a), cc = std::cos(c), sc = std::sin(c);
    const double Q[9] = {ca, -sa * cc, sa * sc, sa, ca * cc, -ca * sc, 0.0, sc, cc};
    const double sv[3] = {1.0, 6.0, 30.0};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) T[(size_t)k * 9 + i * 3 + j] = sv[i] * Q[i * 3 + j];
  }
  // block (k, l) = L_kl T_k^T T_l, entry (i, j) = L_kl sum_q T_k[q, i] T_l[q, j]
  auto entry = [&](int k, int l, int i, int j, double lkl) {
    double s = 0.0;
    for (int q = 0; q < 3; ++q) s += T[(size_t)k * 9 + q * 3 + i] * T[(size_t)l * 9 + q * 3 + j];
    return lkl * s;
  };
  std::vector<int> rowptr(1, 0), col, rowof;
  std::vector<double> val;
  for (int k = 0; k < nn; ++k) {
    const int x = k % nx, y = k / nx;
    const int nb[5] = {y > 0 ? k - nx : -1, x > 0 ? k - 1 : -1, k, x < nx - 1 ? k + 1 : -1,
                       y < ny - 1 ? k + nx : -1};
    for (int i = 0; i < bs; ++i) {
      for (int l : nb) {
        if (l < 0) continue;
        for (int j = 0; j < bs; ++j) {
          double v;
          if (l == k)  // the upper triangle, mirrored: exactly symmetric
            v = i <= j ? entry(k, k, i, j, 4.0) : entry(k, k, j, i, 4.0);
          else  // the block above the diagonal, mirrored as its transpose
            v = l > k ? entry(k, l, i, j, -1.0) : entry(l, k, j, i, -1.0);
          col.push_back(l * bs + j);
          val.push_back(v);
        }
      }
      rowptr.push_back((int)col.size());
      rowof.resize(col.size(), k * bs + i);
    }
  }
  const size_t nnz = val.size(), len = (size_t)nsys * n;
  std::vector<double> vals(nsys * nnz), B(len);
  double nb2 = 0;
  for (int i = 0; i < n; ++i) nb2 += (1.0 + i % 7) * (1.0 + i % 7);
  for (int s = 0; s < nsys; ++s) {
    auto d = [&](int i) { return std::pow(10.0, s * ((7 * i) % 11) / (44.0 * nsys)); };
    for (size_t e = 0; e < nnz; ++e) vals[s * nnz + e] = d(rowof[e]) * val[e] * d(col[e]);
    for (int i = 0; i < n; ++i) B[(size_t)s * n + i] = 1.0 + i % 7;
  }
  const double tol = 1e-8 * std::sqrt(nb2);

  acpp::sycl::queue q;
  CGMany<double> many(q, rowptr, col, vals);
  auto all_by_rule = [&] {
    for (int c : many.stopped())
      if (c != 1) return false;
    return true;
  };
  auto total = [&] {
    long long t = 0;
    for (int64_t b : many.iterations()) t += b;
    return t;
  };
  std::vector<double> Xj(len, 0.0), Xb(len, 0.0), Xg(len, 0.0);
  many.setPreconditioner(CGX_PRECOND_JACOBI);
  many.solve(B, Xj, tol);
  bool ok = true;
  const long long jac = total();

  many.setBlockPreconditioner(CGX_BLOCK_JACOBI, bs);
  ok = ok && many.preconditioner() == CGX_PRECOND_NONE &&
       many.blockPreconditioner() == CGX_BLOCK_JACOBI;
  many.solve(B, Xb, tol);
  ok = ok && all_by_rule();
  const long long blk = total();
  const std::vector<int64_t> blk_bodies = many.iterations();
  const std::vector<double> blk_rr = many.finalResidualSquared(), blk_rz = many.finalRz();

  int64_t bad = -1;
  const std::vector<double> W = many.blockInverse(bs, &bad);
  many.setBlockPreconditioner(CGX_BLOCK_GIVEN, bs, &W);
  many.solve(B, Xg, tol);
  ok = ok && all_by_rule() && bad == 0;
  const bool same = std::memcmp(Xg.data(), Xb.data(), len * sizeof(double)) == 0 &&
                    many.iterations() == blk_bodies &&
                    std::memcmp(many.finalResidualSquared().data(), blk_rr.data(),
                                nsys * sizeof(double)) == 0 &&
                    std::memcmp(many.finalRz().data(), blk_rz.data(), nsys * sizeof(double)) == 0;
  const bool fewer = blk < jac;
  ok = ok && same && fewer;
  std::printf("many_block_pcg_check: %d systems of n = %d, bs = %d; JACOBI and GIVEN from "
              "blockInverse %s; bodies Jacobi %lld, block-Jacobi %lld: %s; %s\n",
              nsys, n, bs, same ? "agree bit for bit" : "DIFFER", jac, blk,
              fewer ? "fewer bodies" : "NOT fewer", ok ? "agreement" : "NO agreement");
  return ok ? 0 : 1;
}
