// fixed_msm_long_plan.hpp -- how d377_batch_fixed_long_msm (fixed_bases.hip) cuts a fixed-base sum over m registered bases into
// segments of consecutive bases, one lane per segment.  Plain integer arithmetic, shared by the host code, the kernel and the
// host simulation (tests/host_sim/fixed_msm_long_sim.cpp), like batch_msm_long_plan.hpp, whose fold (fold_out, fold_count,
// BML_FOLD) adds the segments' partial sums.
//
//   L   = resident lanes of the device (CUs x WAVES_PER_SIMD x BLOCK: 131 072 on 256 CUs)
//   cap = ceil(L / n)                            segments per sum that fill the chip once
//   g0  = min(ceil(m / FML_SEG_MIN), cap)        FML_SEG_MIN: fewest bases worth a segment
//   b   = ceil(m / g0),  g = ceil(m / b)         segment q covers the bases [q b, min(m, (q + 1) b)): none is empty, the last may
//                                                be shorter
//
// Rounding b up can leave far fewer than g0 segments (m = 1042, g0 = 1041: b = 2, g = 521 -- half the chip).  Where it loses
// more than one segment per sum against what fills the chip, n g < min(L, n ceil(m / FML_SEG_MIN)) - n, b is rounded down
// instead (b - 1 >= 1 there, and ceil(m / (b - 1)) >= g0): the lanes then overshoot L, and the grid-stride kernel walks the
// few extra segments in a second pass.  n >= L or m = 1 gives g = 1: the caller runs the one-lane-per-sum kernel.
// g <= m <= 4096 is at most three fold levels (4096 -> 256 -> 16 -> 1).
#pragma once
#include <stddef.h>

#include "batch_msm_long_plan.hpp"

#ifndef D377_FML_SEG_MIN
#define D377_FML_SEG_MIN 1
#endif

namespace d377 {

constexpr size_t FML_SEG_MIN = D377_FML_SEG_MIN;

struct FixedLongPlan {
  size_t m, g, b;                        // bases per sum, segments per sum, bases per segment (the last may hold fewer)
  D377_BML_HD size_t first(size_t q) const { return q * b; }                                 // segment q's first base
  D377_BML_HD size_t count(size_t q) const { return m - q * b < b ? m - q * b : b; }          // its bases: 1 .. b
};
// n >= 1 sums over m >= 1 bases on a device of L >= 1 resident lanes
D377_BML_HD FixedLongPlan fixed_long_plan(size_t m, size_t n, size_t L) {
  FixedLongPlan p;
  p.m = m;
  if (n >= L) { p.g = 1; p.b = m; return p; }                  // (and n x m below stays far from overflow)
  const size_t cap = (L + n - 1) / n, most = (m + FML_SEG_MIN - 1) / FML_SEG_MIN;
  const size_t g0 = most < cap ? most : cap;
  p.b = (m + g0 - 1) / g0;
  p.g = (m + p.b - 1) / p.b;
  const size_t fill = L < n * most ? L : n * most;
  if (n * p.g + n < fill) {              // (b >= 2 here: b = 1 is g = m >= most)
    p.b -= 1;
    p.g = (m + p.b - 1) / p.b;
  }
  return p;
}

}  // namespace d377
