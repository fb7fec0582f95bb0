// msm_ragged_plan.hpp -- the integer plan of d377_batch_ragged_msm (msm_ragged.inc): many sums of ANY length each, delimited by
// n + 1 offsets into the term-major arrays, through the bucket pipeline of d377_batch_bucket_msm (msm_batch_plan.hpp).  Behind
// the composite keys no stage of that pipeline knows which term belongs to which sum, so a sum's length enters in two places
// only, both here:
//   the lookup     term g -> its sum, by a search over the offsets of the pass (rsum_sum_of_term; the keys kernel narrows it
//                  per 256-term tile, rsum_tile_sum);
//   the pass cut   greedy runs of consecutive sums: a pass takes the next sum while (K + 1) 2^(c-1) <= 2^17 (the sort's table,
//                  BSUM_MAX_KEYS) and points + length <= 2^24 (the packed placement, BSUM_MAX_POINTS).  A length is at most
//                  2^20, so every sum fits a pass.  msm_plan runs per pass with n = the points of the pass and sums = K; a pass
//                  without a point never enters the pipeline (msm_plan is not asked about n = 0).
// With equal lengths the cut, the width and the bytes are bsum_plan's.
// THE WINDOW WIDTH is bsum_window of the MEAN length, max(1, ceil(terms / n)): the uniform call's rule applied to the one
// statistic that makes the two calls agree on equal lengths.  Whether the mean is the right statistic for skewed lengths has
// not been measured (tools/bench_ragged_sums.py sweeps window_bits on a skewed shape; DESIGN.md 4.4b keeps the open item).
// Plain integer code shared by the kernel, the launcher and the host simulation (tests/host_sim/ragged_sums_sim.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "msm_batch_plan.hpp"

namespace d377 {

constexpr size_t RSUM_MAX_TERMS = BSUM_MAX_TERMS;      // D377_BATCH_RAGGED_MSM_MAX_TERMS, per sum
constexpr int RSUM_TILE = 256;                         // terms per workgroup of k_rsum_keys

// The largest k in lo .. hi with off[k] <= g, or lo if there is none (or if lo > hi).  The result lies in lo .. max(lo, hi)
// for ANY array contents: the search never leaves the interval it was given.
D377_HD uint32_t rsum_search(const uint64_t* off, uint32_t lo, uint32_t hi, uint64_t g) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1u) / 2u;
    if (off[mid] <= g) lo = mid; else hi = mid - 1u;
  }
  return lo;
}
// Term g -> its sum among the K >= 1 sums whose offsets are off[0 .. K]: the largest k < K with off[k] <= g, so a run of equal
// offsets (empty sums) before a non-empty sum resolves to that non-empty sum.  Clamped to 0 .. K - 1 whatever the array holds
// and whatever g is: off[K] is never read.
D377_HD uint32_t rsum_sum_of_term(const uint64_t* off, uint32_t K, uint64_t g) { return rsum_search(off, 0u, K - 1u, g); }
// What a lane of k_rsum_keys does for pass-local term i of n (term base + i of the call): the sums of the first and the last
// term of its 256-term tile bound the search (both the same for every lane of the workgroup), 0 - 2 steps inside long sums and
// at most 8 where every term is a sum of its own.  Equal to rsum_sum_of_term(off, K, base + i) when the offsets are monotone;
// in 0 .. K - 1 always.
D377_HD uint32_t rsum_tile_sum(const uint64_t* off, uint32_t K, uint64_t base, size_t n, size_t i) {
  const size_t i0 = i - i % (size_t)RSUM_TILE, i1 = i0 + RSUM_TILE - 1 < n ? i0 + RSUM_TILE - 1 : n - 1;
  return rsum_search(off, rsum_sum_of_term(off, K, base + i0), rsum_sum_of_term(off, K, base + i1), base + i);
}

// The first sum whose offsets are at fault -- off[i + 1] < off[i], or a length above RSUM_MAX_TERMS -- or n if there is none.
inline size_t rsum_first_bad_sum(const uint64_t* off, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i] || off[i + 1] - off[i] > RSUM_MAX_TERMS) return i;
  return n;
}

// the width of a call of n sums and `terms` terms
inline int rsum_window(uint64_t terms, size_t n, int window_bits) {
  if (window_bits) return window_bits;
  const uint64_t sums = n < 1 ? 1 : n;
  const uint64_t mean = (terms + sums - 1) / sums;
  return bsum_window((size_t)(mean < 1 ? 1 : mean));
}

// The pass that begins at sum `first` < n: `sums` >= 1 consecutive sums holding `points` terms.
struct RsumPass { size_t first, sums, points; };
inline RsumPass rsum_next_pass(const uint64_t* off, size_t n, size_t first, int c) {
  RsumPass p{first, 0, 0};
  while (first + p.sums < n && ((p.sums + 1) << (c - 1)) <= BSUM_MAX_KEYS) {
    const size_t len = (size_t)(off[first + p.sums + 1] - off[first + p.sums]);
    if (p.points + len > BSUM_MAX_POINTS) break;
    p.points += len; ++p.sums;
  }
  return p;
}
inline MsmPlan rsum_pass_plan(const RsumPass& ps, int c, int cus, int span_blocks) {
  MsmPlanIn in;
  in.n = ps.points; in.c = c; in.cus = cus; in.span_blocks = span_blocks; in.sums = ps.sums;
  return msm_plan(in);
}

// The plan of a call: the width, the passes, the largest pass by sums and by points, and the workspace: the largest `bytes` of
// the passes that hold a point (0 when none does).
struct RsumPlan {
  int c;
  size_t passes, max_sums, max_points, bytes;
};
inline RsumPlan rsum_plan(const uint64_t* off, size_t n, int window_bits, int cus, int span_blocks) {
  RsumPlan p{};
  p.c = rsum_window(n ? off[n] - off[0] : 0, n, window_bits);
  size_t seen_sums = 0, seen_points = 0, seen_bytes = 0;         // (most passes of a call repeat the shape of the one before)
  for (size_t first = 0; first < n;) {
    const RsumPass ps = rsum_next_pass(off, n, first, p.c);
    ++p.passes;
    if (ps.sums > p.max_sums) p.max_sums = ps.sums;
    if (ps.points > p.max_points) p.max_points = ps.points;
    if (ps.points) {
      if (ps.sums != seen_sums || ps.points != seen_points) {
        seen_sums = ps.sums; seen_points = ps.points;
        seen_bytes = rsum_pass_plan(ps, p.c, cus, span_blocks).bytes;
      }
      if (seen_bytes > p.bytes) p.bytes = seen_bytes;
    }
    first += ps.sums;
  }
  return p;
}

// The host forms' slices over `devices` devices: cut k (0 .. devices) is the sum boundary whose offset is nearest to the equal
// share of TERMS, floor(terms k / devices) past off[0] -- the lower boundary on a tie or among equal offsets; cut 0 is 0 and cut
// `devices` is n.  Device k takes the sums cut k .. cut k+1 - 1.  The cuts never decrease.
inline size_t rsum_device_cut(const uint64_t* off, size_t n, size_t devices, size_t k) {
  if (k == 0 || n == 0) return 0;
  if (k >= devices) return n;
  const uint64_t terms = off[n] - off[0];
  const uint64_t target = off[0] + terms / devices * k + terms % devices * k / devices;   // floor(terms k / devices), no overflow
  size_t lo = 0, hi = n;                                         // the first boundary with off[j] >= target
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    if (off[mid] < target) lo = mid + 1; else hi = mid;
  }
  if (lo > 0 && target - off[lo - 1] <= off[lo] - target) {      // the boundary below is as near or nearer ...
    const uint64_t v = off[lo - 1];
    --lo;
    while (lo > 0 && off[lo - 1] == v) --lo;                      // ... and the first of its equals
  }
  return lo;
}

}  // namespace d377
