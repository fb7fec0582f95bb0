// msm_segmented_plan.hpp -- the integer plan of d377_batch_segmented_msm (batch_msm_segmented.hip): many sums of ANY length
// each, delimited by n + 1 offsets into the term-major arrays, by the Straus chains of d377_batch_msm_long.  Plain integer
// arithmetic, shared by the host code, the kernels and the host simulation (tests/host_sim/segmented_sums_sim.cpp), like
// batch_msm_long_plan.hpp.
//
//   the cut        sum i of length L has long_plan(L)'s cut: g = ceil(L / 8) chains of b = ceil(L / g) slots, chain q covers
//                  count(q) live terms from offsets[i] + q b (L = 9: 5 + 4).  An empty sum has no chain.
//   the slots      no prefix scan and no table built on the host: the chains of sum i lie from slot
//                      start_0(i) = floor((offsets[i] - offsets[0]) / 8) + i
//                  of a space of S_0 = floor(T / 8) + n records, T the number of terms.  Since
//                  floor((o + L) / 8) - floor(o / 8) + 1 >= ceil(L / 8), the g slots of sum i end before those of sum i + 1
//                  begin; the starts increase STRICTLY, so a run of empty sums is no special case.  At most n slots are dead.
//   the lookup     the lane or wave of slot p finds its sum by binary search on start (seg_find), takes q = p - start(i) and is
//                  live iff q < g.
//   the fold       the same step again: level l + 1 places sum i at start_{l+1}(i) = floor(start_l(i) / 16) + i in a space of
//                  S_{l+1} = floor(S_l / 16) + n records, where it has fold_out(c_i) records for its c_i of level l.  The
//                  slot-indexed levels run while some sum has more than 16 records (their number comes from the longest sum);
//                  a last, sum-indexed level adds a sum's <= 16 records into record i of a compact array.
// EVERY LOOKUP IS CLAMPED: seg_find answers in 0 .. n - 1 whatever the array holds, a length is cut at SEG_MAX_TERMS, a chain
// reads no term from T on and a fold lane no record from S_l on (T and S_l come from the HOST offsets, by value).  Offsets on the
// device that differ from the host's give wrong sums and safe memory.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "batch_msm_long_plan.hpp"

namespace d377 {

constexpr uint64_t SEG_MAX_TERMS = 1u << 20;           // D377_BATCH_SEGMENTED_MSM_MAX_TERMS, per sum
constexpr int SEG_MAX_LEVELS = 4;                      // slot-indexed fold levels: 2^17 chains -> 8192 -> 512 -> 32 -> 2 (the last level adds those)
// advised_route: chains (0) while the mean length of the NON-EMPTY sums is below this, buckets (1) from it on.  Set by
// measurement (profiles/segmented_sums_bench.json, tools/bench_segmented_sums.py): equal lengths 512 .. 1024 at 2^20 terms
// per call, d377_batch_long_msm_resident against d377_batch_bucket_msm_resident; 1024 is the smallest length at which the
// buckets lead by more than the two spreads together (6.595 against 7.088 ms; at 896 the medians lie inside the spreads).
// ESTABLISHED BY THAT SWEEP; it is also the point the project had measured before (6.55 against 7.04 ms).
constexpr uint64_t SEG_CHAINS_BELOW_MEAN = 1024;

// the length of sum i as the device reads it: cut at the limit, so that a decrease (a wrapped difference) stays bounded
D377_BML_HD uint64_t seg_len(const uint64_t* off, size_t i) {
  const uint64_t L = off[i + 1] - off[i];
  return L < SEG_MAX_TERMS ? L : SEG_MAX_TERMS;
}
D377_BML_HD size_t seg_chains(uint64_t L) { return (size_t)((L + BML_GROUP_MAX - 1) / BML_GROUP_MAX); }
// records of a sum of length L at fold level `level` (0: its chains)
D377_BML_HD size_t seg_records(uint64_t L, int level) {
  size_t c = seg_chains(L);
  for (int l = 0; l < level; ++l) c = fold_out(c);
  return c;
}
// slot-indexed levels of a call whose longest sum has max_len terms: fold while some sum has more than BML_FOLD records
D377_BML_HD int seg_levels(uint64_t max_len) {
  int levels = 0;
  for (size_t c = seg_chains(max_len); c > BML_FOLD; c = fold_out(c)) ++levels;
  return levels;
}
// the first slot of sum i at `level`
D377_BML_HD uint64_t seg_start(const uint64_t* off, size_t i, int level) {
  uint64_t s = (off[i] - off[0]) / BML_GROUP_MAX + i;
  for (int l = 0; l < level; ++l) s = s / BML_FOLD + i;
  return s;
}
// the slots of `level` for T terms in n sums
D377_BML_HD size_t seg_space(uint64_t T, size_t n, int level) {
  size_t S = (size_t)(T / BML_GROUP_MAX) + n;
  for (int l = 0; l < level; ++l) S = S / BML_FOLD + n;
  return S;
}
// Slot p of `level` -> its sum among n >= 1: the largest i < n with start(i) <= p, or 0 if there is none.  In 0 .. n - 1 for
// ANY array contents: the search never leaves its interval, and off[n] is not read.
D377_BML_HD size_t seg_find(const uint64_t* off, size_t n, int level, uint64_t p) {
  size_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo + 1) / 2;
    if (seg_start(off, mid, level) <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// What the lane or wave of chain slot p does: live = false, or the chain's first term (past off[0]) and its live terms.  T: the
// terms of the call by the HOST offsets; bmax: the slots the table scratch holds per lane.
struct SegChain {
  bool live;
  size_t sum, q;
  uint64_t first;                        // relative to off[0]
  int count, b;                          // live terms 1 .. b; slots of the sum's chains
};
D377_BML_HD SegChain seg_chain(const uint64_t* off, size_t n, uint64_t T, int bmax, uint64_t p) {
  SegChain c;
  c.live = false; c.first = 0; c.count = 0; c.b = 0;
  c.sum = seg_find(off, n, 0, p);
  c.q = (size_t)(p - seg_start(off, c.sum, 0));
  const uint64_t L = seg_len(off, c.sum);
  if (L == 0) return c;                                           // (long_plan divides by g)
  const LongPlan lp = long_plan((size_t)L);
  if (c.q >= lp.g) return c;
  c.first = (off[c.sum] - off[0]) + (uint64_t)(c.q * lp.b);
  if (c.first >= T) return c;                                     // (only with offsets that differ from the host's)
  uint64_t cnt = lp.count(c.q);
  if (cnt > T - c.first) cnt = T - c.first;
  c.b = (int)lp.b < bmax ? (int)lp.b : bmax;
  c.count = (int)cnt < c.b ? (int)cnt : c.b;
  c.live = true;
  return c;
}

// What the lane of slot p of level `level` + 1 does: dead, or add `count` records of level `level` from record `lo`.
// S_in: the slots of level `level` by the HOST offsets.
struct SegFold {
  bool live;
  size_t sum;
  uint64_t lo;
  int count;
};
D377_BML_HD SegFold seg_fold(const uint64_t* off, size_t n, int level, size_t S_in, uint64_t p) {
  SegFold f;
  f.live = false; f.lo = 0; f.count = 0;
  f.sum = seg_find(off, n, level + 1, p);
  const uint64_t j = p - seg_start(off, f.sum, level + 1);
  const size_t c = seg_records(seg_len(off, f.sum), level);
  if (j >= fold_out(c)) return f;
  f.lo = seg_start(off, f.sum, level) + j * BML_FOLD;
  if (f.lo >= S_in) return f;
  uint64_t cnt = fold_count(c, (size_t)j);
  if (cnt > S_in - f.lo) cnt = S_in - f.lo;
  f.count = (int)cnt;
  f.live = true;
  return f;
}
// The last level, lane i: the 0 .. BML_FOLD records of sum i at level `levels`; count == 0 is an empty sum.
D377_BML_HD SegFold seg_last(const uint64_t* off, size_t i, int levels, size_t S_in) {
  SegFold f;
  f.sum = i;
  f.lo = seg_start(off, i, levels);
  uint64_t cnt = seg_records(seg_len(off, i), levels);
  if (cnt > BML_FOLD) cnt = BML_FOLD;
  if (f.lo >= S_in) cnt = 0;
  else if (cnt > S_in - f.lo) cnt = S_in - f.lo;
  f.count = (int)cnt;
  f.live = cnt != 0;
  return f;
}

// The plan of a call, from the host offsets (checked: monotone, every length within the limit).
struct SegPlan {
  uint64_t terms;
  size_t chain_slots, chains, max_len;
  int levels, bmax;                      // slot-indexed fold levels; the most slots of a chain (0 when no sum has a term)
  size_t space[SEG_MAX_LEVELS + 1];      // slots of level 0 .. levels
  size_t base[SEG_MAX_LEVELS + 2];       // the first record of level l in the area; base[levels + 1]: the n compact records
  size_t records;                        // of the whole area
  int advised_route;                     // 0 chains, 1 buckets
};
inline SegPlan seg_plan(const uint64_t* off, size_t n) {
  SegPlan p{};
  if (n == 0) return p;
  p.terms = off[n] - off[0];
  size_t nonempty = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint64_t L = off[i + 1] - off[i];
    if (!L) continue;
    ++nonempty;
    const LongPlan lp = long_plan((size_t)L);
    p.chains += lp.g;
    if (L > p.max_len) p.max_len = (size_t)L;
    if ((int)lp.b > p.bmax) p.bmax = (int)lp.b;
  }
  p.levels = seg_levels(p.max_len);
  size_t at = 0;
  for (int l = 0; l <= p.levels; ++l) {
    p.space[l] = seg_space(p.terms, n, l);
    p.base[l] = at;
    at += p.space[l];
  }
  p.base[p.levels + 1] = at;
  p.records = at + n;
  p.chain_slots = p.space[0];
  p.advised_route = (nonempty && p.terms >= SEG_CHAINS_BELOW_MEAN * (uint64_t)nonempty) ? 1 : 0;
  return p;
}

}  // namespace d377
