// cgx_sweep.h — the sweep direction of a CG body's launches (no HIP
// dependency: examples/sweep_check.cpp compiles it with a plain C++ compiler).
#pragma once

namespace cgx {

// Direction (0 low to high, 1 high to low) of launch k of the body in `slot`,
// for a body of `launches_per_body` sweeping launches: the launches alternate
// in stream order, across the body boundary and across slot 3 -> slot 0 too,
// so each launch starts at the end the one before it just left, where the
// vectors they share are newest in L2 and the Infinity Cache (DESIGN.md §5
// "Alternating sweep directions"). Three launches: slot & 1, 1 - (slot & 1),
// slot & 1. Two launches: 0, 1 in every slot. Body 0 starts forward, and four
// slots hold an even number of launches, so the slot's position in its group
// is all the rule needs.
inline int sweep_dir(int launches_per_body, int slot, int k) {
  return (slot * launches_per_body + k) & 1;
}

}  // namespace cgx
