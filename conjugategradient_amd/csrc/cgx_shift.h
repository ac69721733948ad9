// cgx_shift.h — the scalar step of multi-shift CG (cgx_cg_solve_shifted,
// DESIGN.md §5g): what one shift (A + sigma I) x_s = b does with the base
// recurrence's alpha and beta in one body. No HIP dependency when a plain C++
// compiler reads it (examples/shift_step_check.cpp); the kernel
// (cgx_kernels.hip k_update_xp_shift) calls the same function. Build with
// -ffp-contract=off: every operation below is rounded on its own.
#pragma once

#include <cfloat>
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CGX_SHIFT_HD __host__ __device__
#else
#define CGX_SHIFT_HD
#endif

namespace cgx {

constexpr int kShiftMax = 8;  // CGX_SHIFT_MAX (cgx.h)

// One shift's scalars of body n: zn = zeta_{n+1}, as and bs the shift's own
// alpha and beta (x_s += as p_s ; p_s = zn r_{n+1} + bs p_s), stop: the shift
// is frozen after this body.
struct ShiftStep {
  double zn, as, bs;
  bool stop;
};

// a = alpha_n, bt = beta_n, ap = alpha_{n-1}, bp = beta_{n-1} (1 and 0 in body
// 0), zc = zeta_n, zp = zeta_{n-1} (both 1 in body 0), rxr = r.r at the start
// of the body. The parentheses are the evaluation order. With sigma = 0 and
// finite scalars t1 = +0, t2 = ap and zn = 1 exactly, so as = a and bs = bt:
// the single solve.
// Freeze rule (Q5 on the shift's own residual norm |zeta_n| ||r_n||, or a
// zeta that left the normal range: its residual is below DBL_MIN ||r|| and
// the next body would divide 0 by 0; a NaN zeta freezes too).
CGX_SHIFT_HD inline ShiftStep shift_step(double a, double bt, double ap, double bp, double sigma,
                                         double zc, double zp, double rxr, double tol) {
  const double t1 = (a * bp) * (zp - zc);
  const double t2 = (zp * ap) * (1.0 + sigma * a);
  const double zn = ((zc * zp) * ap) / (t1 + t2);
  const double q = zn / zc;
  ShiftStep o;
  o.zn = zn;
  o.as = a * q;
  o.bs = (bt * q) * q;
  o.stop = (rxr != rxr) || std::fabs(zc) * std::sqrt(rxr) <= tol ||
           !(std::fabs(zn) >= DBL_MIN);
  return o;
}

}  // namespace cgx
