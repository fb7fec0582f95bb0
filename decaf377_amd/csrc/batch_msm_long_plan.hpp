// batch_msm_long_plan.hpp -- how d377_batch_msm_long (batch_msm_long.hip) cuts a sum of m > 8 terms into Straus chains and how
// the chains' partial sums are folded.  Plain integer arithmetic, shared by the host code, the kernels and the host
// simulation (tests/host_sim/batch_msm_long_sim.cpp), like msm_plan.hpp.
//
//   g = ceil(m / 8) groups per sum, b = ceil(m / g) <= 8 terms per group; group q covers the terms [q b, min(m, (q + 1) b)).
//   (m = 9: two chains of 5 and 4 terms, not 8 and 1.)  No group is empty: (g - 1) b <= (g - 1) 8 < m.  The slots of the last
//   group past the end of the sum -- fewer than g of them, g b - m < g -- are DEAD: a chain that runs b slots reads nothing for
//   them and they meet only their table's identity entry.
//   Partial sum p = s g + q of sum s is one Element record.  A fold level turns c records per sum into ceil(c / BML_FOLD): one
//   lane adds up to BML_FOLD consecutive records of one sum; the levels repeat until one record per sum is left (g = 512:
//   512 -> 32 -> 2 -> 1).
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define D377_BML_HD __host__ __device__ inline
#else
#define D377_BML_HD inline
#endif

namespace d377 {

constexpr size_t BML_GROUP_MAX = 8;      // terms of one Straus chain (straus.hpp: the eight nibbles of a digit word)
constexpr size_t BML_FOLD = 16;          // records one lane adds in a fold level

struct LongPlan {
  size_t m, g, b;                        // terms per sum, groups per sum, slots per group
  D377_BML_HD size_t first(size_t q) const { return q * b; }                                 // group q's first term within its sum
  D377_BML_HD size_t count(size_t q) const { return m - q * b < b ? m - q * b : b; }          // its live terms: 1 .. b
};
D377_BML_HD LongPlan long_plan(size_t m) {
  LongPlan p;
  p.m = m;
  p.g = (m + BML_GROUP_MAX - 1) / BML_GROUP_MAX;
  p.b = (m + p.g - 1) / p.g;
  return p;
}
// records per sum after one fold level over c records per sum
D377_BML_HD size_t fold_out(size_t c) { return (c + BML_FOLD - 1) / BML_FOLD; }
// output record f of a sum's level adds the records [f BML_FOLD, f BML_FOLD + fold_count(c, f)) of that sum
D377_BML_HD size_t fold_count(size_t c, size_t f) { return c - f * BML_FOLD < BML_FOLD ? c - f * BML_FOLD : BML_FOLD; }

}  // namespace d377
