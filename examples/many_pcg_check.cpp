// many_pcg_check.cpp — the preconditioned many-systems solve
// (CGMany::setPreconditioner, a thin layer over cgx_many_set_precond) from C++:
// a few 2-D Poisson systems on one pattern, system s scaled symmetrically
// D A D with d_i = 10^((s + 1) ((7 i) mod 11) / 55) (up to a decade at the
// last system: badly scaled, which is what Jacobi undoes), solved in one call
//   plain, with Jacobi, and with the caller's diagonal m = 1 / a_ii,
// and one at a time by CG<double>::solve with Preconditioner::Jacobi.
//
//   many_pcg_check [nx ny nsys]      (default 17 15 5; b_i = 1 + (i mod 7))
// Checks, printing one line and returning 0 when all hold, 1 otherwise:
//  - every Jacobi solution agrees with CG::solve's to 1e-7 relative (both
//    residuals are at most 1e-12 ||b||, so the solutions differ by at most
//    2 cond(D A D) 1e-12, and cond(D A D) <= 100 cond(A) < 1.2e4 at the
//    default size);
//  - the caller's diagonal 1 / a_ii gives Jacobi's x, bodies and r.z bit for
//    bit (the same m, read instead of formed);
//  - Jacobi needs fewer bodies than the plain loop, summed over the systems;
//  - with a_00 of system 1 negated, that system alone stops with code 3 and
//    its X untouched, and the others give the bits they gave before.
// Also counts the systems whose x and body count are identical to CG::solve's
// (the bit-for-bit pin to mode 1 is tests/test_gpu_many_pcg.py's).
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
  if (nx < 1 || ny < 1 || nsys < 2) return 2;
  const int n = nx * ny;
  std::vector<int> rowptr(1, 0), col, rowof;
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
      rowof.resize(col.size(), row);
    }
  const size_t nnz = val.size(), len = (size_t)nsys * n;
  std::vector<double> vals(nsys * nnz), B(len), minv(len);
  double nb = 0;
  for (int i = 0; i < n; ++i) nb += (1.0 + i % 7) * (1.0 + i % 7);
  for (int s = 0; s < nsys; ++s) {
    auto d = [&](int i) { return std::pow(10.0, (s + 1.0) * ((7 * i) % 11) / (11.0 * nsys)); };
    for (size_t e = 0; e < nnz; ++e) {
      vals[s * nnz + e] = d(rowof[e]) * val[e] * d(col[e]);
      if (col[e] == rowof[e]) minv[(size_t)s * n + rowof[e]] = 1.0 / vals[s * nnz + e];
    }
    for (int i = 0; i < n; ++i) B[(size_t)s * n + i] = 1.0 + i % 7;
  }
  const double tol = 1e-12 * std::sqrt(nb);

  acpp::sycl::queue q;
  CGMany<double> many(q, rowptr, col, vals);
  std::vector<double> Xp(len, 0.0), Xj(len, 0.0), Xd(len, 0.0);
  many.solve(B, Xp, tol);
  const std::vector<int64_t> plain_bodies = many.iterations();
  bool ok = many.finalRz().empty();
  many.setPreconditioner(CGX_PRECOND_JACOBI);
  many.solve(B, Xj, tol);
  const std::vector<int64_t> jac_bodies = many.iterations();
  const std::vector<double> jac_rz = many.finalRz();
  const std::vector<int> jac_stopped = many.stopped();
  many.setPreconditioner(CGX_PRECOND_DIAGONAL, &minv);
  many.solve(B, Xd, tol);
  const bool diag_same = std::memcmp(Xd.data(), Xj.data(), len * sizeof(double)) == 0 &&
                         many.iterations() == jac_bodies &&
                         std::memcmp(many.finalRz().data(), jac_rz.data(),
                                     nsys * sizeof(double)) == 0;

  int bitwise = 0, agree = 0;
  long long tot_plain = 0, tot_jac = 0;
  double worst = 0;
  for (int s = 0; s < nsys; ++s) {
    std::vector<double> vs(vals.begin() + s * nnz, vals.begin() + (s + 1) * nnz);
    std::vector<double> bs(B.begin() + (size_t)s * n, B.begin() + (size_t)(s + 1) * n);
    std::vector<int> cs = col, rs = rowptr;
    CG<double> cg(q);
    cg.setMatrix(vs, cs, rs);
    cg.setTarget(bs);
    cg.setPreconditioner(Preconditioner::Jacobi);
    cg.solve(tol);
    const std::vector<double> xd = cg.extract();
    const double *xm = Xj.data() + (size_t)s * n;
    double num = 0, den = 0;
    for (int i = 0; i < n; ++i) {
      num += (xm[i] - xd[i]) * (xm[i] - xd[i]);
      den += xd[i] * xd[i];
    }
    const double rel = std::sqrt(num / den);
    if (rel > worst) worst = rel;
    if (rel <= 1e-7 && jac_stopped[s] == 1) ++agree;
    if (std::memcmp(xm, xd.data(), n * sizeof(double)) == 0 && jac_bodies[s] == cg.iterations())
      ++bitwise;
    tot_plain += plain_bodies[s];
    tot_jac += jac_bodies[s];
  }

  // a bad diagonal stops its own system and no other
  const size_t e00 = 0;  // row 0 is (0, 0), (0, 1), (0, nx): its first entry is a_00
  std::vector<double> vbad = vals;
  vbad[nnz + e00] = -vbad[nnz + e00];
  many.setValues(vbad);
  many.setPreconditioner(CGX_PRECOND_JACOBI);
  std::vector<double> Xb(len, -3.5);
  for (int s = 0; s < nsys; ++s)
    if (s != 1) std::fill(Xb.begin() + (size_t)s * n, Xb.begin() + (size_t)(s + 1) * n, 0.0);
  many.solve(B, Xb, tol);
  bool isolated = many.stopped()[1] == 3 && many.iterations()[1] == 0 &&
                  std::isnan(many.finalResidualSquared()[1]) && std::isnan(many.finalRz()[1]);
  for (int s = 0; s < nsys; ++s) {
    const double *xb = Xb.data() + (size_t)s * n;
    if (s == 1) {
      for (int i = 0; i < n; ++i) isolated = isolated && xb[i] == -3.5;
    } else {
      isolated = isolated && many.stopped()[s] == 1 && many.iterations()[s] == jac_bodies[s] &&
                 std::memcmp(xb, Xj.data() + (size_t)s * n, n * sizeof(double)) == 0;
    }
  }

  ok = ok && agree == nsys && diag_same && tot_jac < tot_plain && isolated;
  std::printf("many_pcg_check: %d systems of n = %d, %d agree with CG::solve under Jacobi to 1e-7 "
              "(worst relative difference %.3e), %d identical in x and bodies; diagonal 1/a_ii "
              "%s Jacobi bit for bit; bodies plain %lld, Jacobi %lld; bad diagonal %s: %s\n",
              nsys, n, agree, worst, bitwise, diag_same ? "equals" : "DIFFERS FROM", tot_plain,
              tot_jac, isolated ? "isolated" : "NOT isolated", ok ? "agreement" : "NO agreement");
  return ok ? 0 : 1;
}
