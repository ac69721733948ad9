// The sweep rule of the CG bodies (conjugategradient_amd/csrc/cgx_sweep.h) on
// the host alone: for 1, 2 and 3 launches per body it prints the direction of
// every launch of 16 consecutive bodies (slot = body & 3, as the driver
// enqueues them), one line "L body slot k dir" each, and checks that
// consecutive launches in stream order run in opposite directions, the step
// from slot 3 to slot 0 included, and that three launches per body give
// slot & 1, 1 - (slot & 1), slot & 1. tests/test_cpp_sweep.py compiles and
// runs it and checks the printed table again.
//   g++ -std=c++17 -Iconjugategradient_amd/csrc examples/sweep_check.cpp
#include <cstdio>

#include "cgx_sweep.h"

int main() {
  int bad = 0;
  for (int L = 1; L <= 3; ++L) {
    int last = -1;
    for (int body = 0; body < 16; ++body) {
      const int slot = body & 3;
      for (int k = 0; k < L; ++k) {
        const int d = cgx::sweep_dir(L, slot, k);
        std::printf("%d %d %d %d %d\n", L, body, slot, k, d);
        if (d != 0 && d != 1) ++bad;
        if (last >= 0 && d == last) ++bad;  // stream order: strictly alternating
        last = d;
      }
      if (L == 3) {
        const int par = slot & 1, rpar = 1 - par;
        if (cgx::sweep_dir(3, slot, 0) != par || cgx::sweep_dir(3, slot, 1) != rpar ||
            cgx::sweep_dir(3, slot, 2) != par)
          ++bad;
      }
    }
    if (cgx::sweep_dir(L, 0, 0) != 0) ++bad;  // body 0 starts forward
  }
  if (bad) std::fprintf(stderr, "sweep_check: %d violations\n", bad);
  return bad ? 1 : 0;
}
