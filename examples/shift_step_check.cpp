// shift_step_check.cpp — the scalar step of multi-shift CG (cgx_shift.h, the
// function the kernel calls) on the host: zeta sequences from recorded base
// scalars, for the test to compare with its model bit for bit
// (tests/test_shift_cpu.py). Host only: no libcgx, no HIP. Build with
// -ffp-contract=off.
//
//   shift_step_check in.bin
// in.bin : int64 bodies, int64 shifts, f64 alpha[bodies], f64 beta[bodies],
//          f64 rxr[bodies] (r.r at the start of each body), f64 sigma[shifts],
//          f64 tol
// stdout : one line per shift: the bit patterns of zeta_{n+1} of every body the
//          shift ran (it stops after the body that freezes it), 16 hex digits
//          each, then "stop" or "run"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cgx_shift.h"

template <class T> static void rd(FILE *f, T *p, size_t n) {
  if (std::fread(p, sizeof(T), n, f) != n) {
    std::fprintf(stderr, "short read\n");
    std::exit(2);
  }
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t nb = 0, ns = 0;
  rd(f, &nb, 1);
  rd(f, &ns, 1);
  std::vector<double> alpha(nb), beta(nb), rxr(nb), sigma(ns);
  double tol = 0;
  rd(f, alpha.data(), alpha.size());
  rd(f, beta.data(), beta.size());
  rd(f, rxr.data(), rxr.size());
  rd(f, sigma.data(), sigma.size());
  rd(f, &tol, 1);
  std::fclose(f);
  for (int64_t s = 0; s < ns; ++s) {
    double ap = 1.0, bp = 0.0, zc = 1.0, zp = 1.0;
    bool stop = false;
    for (int64_t n = 0; n < nb && !stop; ++n) {
      const cgx::ShiftStep o =
          cgx::shift_step(alpha[n], beta[n], ap, bp, sigma[s], zc, zp, rxr[n], tol);
      uint64_t bits;
      std::memcpy(&bits, &o.zn, sizeof(bits));
      std::printf("%016llx ", (unsigned long long)bits);
      zp = zc;
      zc = o.zn;
      ap = alpha[n];
      bp = beta[n];
      stop = o.stop;
    }
    std::printf("%s\n", stop ? "stop" : "run");
  }
  return 0;
}
