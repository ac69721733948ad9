// many_wave_check.cpp — the two forms of the many-systems solve
// (CGMany::setForm, a thin layer over cgx_many_set_form) from C++: a few 2-D
// Poisson systems on one pattern, system s scaled symmetrically D A D with
// d_i = 10^((s + 1) ((7 i) mod 11) / (22 nsys)) (up to half a decade at the
// last system), solved in one call
//   by a workgroup per system and by a wave per system,
//   plain and with Jacobi.
//
//   many_wave_check [nx ny nsys]      (default 9 7 7; b_i = 1 + (i mod 7))
// n = nx ny must be at most 256, the most one wave holds. With n <= 64 the two
// forms give the same bits by construction (cgx.h); above, they do wherever
// the dots are clear of a rounding boundary, which these systems are not
// checked for, so pass sizes above 64 to look, not to test.
// Prints one line and returns 0 when x, the body counts, r.r (and r.z under
// Jacobi) of the two forms are identical and every system stopped by the rule,
// 1 otherwise.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "CGMany.hpp"

using namespace CGSolver;

namespace {
struct Result {
  std::vector<double> X, rxr, rz;
  std::vector<int64_t> bodies;
  std::vector<int> stopped;
};

Result run(CGMany<double> &many, int form, const std::vector<double> &B, double tol) {
  Result r;
  many.setForm(form);
  r.X.assign(B.size(), 0.0);
  many.solve(B, r.X, tol);
  r.rxr = many.finalResidualSquared();
  r.rz = many.finalRz();
  r.bodies = many.iterations();
  r.stopped = many.stopped();
  return r;
}

bool same_bits(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() &&
         (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0);
}
}  // namespace

int main(int argc, char **argv) {
  const int nx = argc > 3 ? std::atoi(argv[1]) : 9, ny = argc > 3 ? std::atoi(argv[2]) : 7;
  const int nsys = argc > 3 ? std::atoi(argv[3]) : 7;
  if (nx < 1 || ny < 1 || nsys < 1 || nx * ny > 256) return 2;
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
  std::vector<double> vals(nsys * nnz), B(len);
  double nb = 0;
  for (int i = 0; i < n; ++i) nb += (1.0 + i % 7) * (1.0 + i % 7);
  for (int s = 0; s < nsys; ++s) {
    auto d = [&](int i) { return std::pow(10.0, (s + 1.0) * ((7 * i) % 11) / (22.0 * nsys)); };
    for (size_t e = 0; e < nnz; ++e) vals[s * nnz + e] = d(rowof[e]) * val[e] * d(col[e]);
    for (int i = 0; i < n; ++i) B[(size_t)s * n + i] = 1.0 + i % 7;
  }
  const double tol = 1e-10 * std::sqrt(nb);

  acpp::sycl::queue q;
  CGMany<double> many(q, rowptr, col, vals);
  bool ok = true, plain_same = false, jacobi_same = false;
  long long bodies[2] = {0, 0};
  for (int pc = 0; pc < 2; ++pc) {
    many.setPreconditioner(pc ? CGX_PRECOND_JACOBI : CGX_PRECOND_NONE);
    const Result wg = run(many, CGX_MANY_FORM_WORKGROUP, B, tol);
    ok = ok && many.form() == CGX_MANY_FORM_WORKGROUP;
    const Result wv = run(many, CGX_MANY_FORM_WAVE, B, tol);
    ok = ok && many.form() == CGX_MANY_FORM_WAVE;
    const bool same = same_bits(wg.X, wv.X) && wg.bodies == wv.bodies &&
                      same_bits(wg.rxr, wv.rxr) && same_bits(wg.rz, wv.rz) &&
                      wg.stopped == wv.stopped && wg.rz.size() == (pc ? (size_t)nsys : 0);
    (pc ? jacobi_same : plain_same) = same;
    for (int s = 0; s < nsys; ++s) {
      ok = ok && wv.stopped[s] == 1;
      bodies[pc] += wv.bodies[s];
    }
  }
  many.setForm(CGX_MANY_FORM_AUTO);
  const int auto_form = many.form();
  ok = ok && plain_same && jacobi_same &&
       (auto_form == CGX_MANY_FORM_WORKGROUP || auto_form == CGX_MANY_FORM_WAVE);
  std::printf("many_wave_check: %d systems of n = %d; workgroup and wave form, x, bodies and r.r: "
              "plain %s (%lld bodies), Jacobi %s (%lld bodies, r.z too); auto takes the %s form: "
              "%s\n",
              nsys, n, plain_same ? "identical" : "DIFFERENT", bodies[0],
              jacobi_same ? "identical" : "DIFFERENT", bodies[1],
              auto_form == CGX_MANY_FORM_WAVE ? "wave" : "workgroup",
              ok ? "agreement" : "NO agreement");
  return ok ? 0 : 1;
}
