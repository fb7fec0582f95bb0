// msm_batch_plan.hpp -- the integer plan of d377_batch_bucket_msm (msm_batch.inc): MANY sums of m terms each through ONE run of
// the bucket method's sort / span / bucket pipeline (msm.hip), by a composite bucket key.
//
// A pass holds K sums of m terms, N = K m points; point i belongs to sum k = i / m.  With c-bit windows its signed digit d of
// window w (msm_digit, on k / 2 mod r as in d377_msm) becomes the key  sign(d) * (k 2^(c-1) + |d|)  (0 stays 0: the pipeline
// skips it).  msm_digit gives |d| <= 2^(c-1) and never +2^(c-1), so the keys of sum k lie in k 2^(c-1) + 1 .. (k + 1) 2^(c-1),
// the top one reached by negative digits only -- the range shape of a single sum -- and a window has nb' = K 2^(c-1) + 1
// buckets.  Bucket j >= 1 belongs to sum (j - 1) >> (c-1) with weight ((j - 1) & (2^(c-1) - 1)) + 1.  After k_msm_buckets the
// bucket records are W K "pseudo-windows" of 2^(c-1) leaves: the tree of bit-sums runs once per pseudo-window and a Horner
// chain per sum finishes.  msm_plan (msm_plan.hpp) with `sums = K` is the plan of one pass.
//
// Limits: the sort's super-bucket table holds 1 025 entries (msm.hip: MAX_SUPER), so K 2^(c-1) <= 2^17; keys travel as int16
// while K 2^(c-1) <= 2^15 (-2^15 is the one key of that magnitude) and as int32 above; the packed placement needs N <= 2^24.
// Plain integer code shared by the kernels, the launcher and the host simulation (tests/host_sim/bucket_sums_sim.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "msm_plan.hpp"

namespace d377 {

constexpr size_t BSUM_MAX_TERMS = (size_t)1 << 20;     // D377_BATCH_BUCKET_MSM_MAX_TERMS
constexpr int BSUM_MIN_WINDOW = 4, BSUM_MAX_WINDOW = 16;   // 16: the 15-deep tree without a middle level
constexpr size_t BSUM_MAX_KEYS = (size_t)1 << 17;      // K 2^(c-1) at most
constexpr size_t BSUM_MAX_POINTS = PACKED_MAX_POINTS;   // K m at most

// digit d of sum k -> the pipeline's digit
D377_HD int bsum_key(uint32_t k, int c, int d) {
  if (d == 0) return 0;
  const int key = (int)(k << (c - 1)) + (d < 0 ? -d : d);
  return d < 0 ? -key : key;
}
// ... and back: the sum and the digit of a non-zero key
D377_HD int bsum_key_digit(int key, int c, uint32_t* k) {
  const uint32_t j = (uint32_t)(key < 0 ? -key : key) - 1u;
  const int a = (int)(j & ((1u << (c - 1)) - 1u)) + 1;
  *k = j >> (c - 1);
  return key < 0 ? -a : a;
}
// bucket j >= 1 of a window: its sum and its weight; the first bucket record of pseudo-window (w, k) less one (leaf i of the
// tree is record base + 1 + i)
D377_HD uint32_t bsum_bucket_sum(uint32_t j, int c) { return (j - 1u) >> (c - 1); }
D377_HD uint32_t bsum_bucket_weight(uint32_t j, int c) { return ((j - 1u) & ((1u << (c - 1)) - 1u)) + 1u; }
D377_HD size_t bsum_leaf_base(int w, size_t k, int nb, int c) { return (size_t)w * (size_t)nb + (k << (c - 1)); }

// THE WINDOW WIDTH, a function of m alone: the width in 4 .. 16 that minimises W(c) (m + BSUM_COST_BUCKET 2^(c-1) +
// BSUM_COST_WINDOW), the narrower on a tie.  By additions alone the weights would be 2 per bucket (the tree of bit-sums) and
// nothing per window, which gives 6 / 9 / 12 / 16 bits at m = 256 / 4096 / 2^16 / 2^20.  The sweep over window_bits on one
// MI355X (profiles/bucket_sums_window_sweep.txt, 2^20 terms per call) has 6 bits ahead at m = 256 (17.6 ms; 5 bits 19.2, 7 bits
// 17.8), 8 ahead at 4096 (3.36 ms against 3.60 at 9), 11 and 12 within each other's spread at 2^16 (2.09 / 2.15 ms), and
// d377_msm's own sweep has 14 ahead of 16 at 2^20 points (msm.hip, pick_window): a bucket costs more than its two additions
// (the sort's counters, offsets and an empty record per bucket, a lane of k_msm_buckets) and every (window, sum) pair a
// workgroup of the tree and a Horner step.  The two weights are fitted to those four points, in units of one addition.
constexpr unsigned long long BSUM_COST_BUCKET = 9, BSUM_COST_WINDOW = 400;
inline int bsum_window(size_t m) {
  int best = BSUM_MIN_WINDOW;
  unsigned long long cost = ~0ull;
  for (int c = BSUM_MIN_WINDOW; c <= BSUM_MAX_WINDOW; ++c) {
    const unsigned long long v = (unsigned long long)win_shape(c).W * ((unsigned long long)m + (BSUM_COST_BUCKET << (c - 1)) + BSUM_COST_WINDOW);
    if (v < cost) { cost = v; best = c; }
  }
  return best;
}
// sums per pass
inline size_t bsum_sums_per_pass(size_t n, size_t m, int c) {
  size_t k = BSUM_MAX_KEYS >> (c - 1);
  const size_t by_points = BSUM_MAX_POINTS / m > 1 ? BSUM_MAX_POINTS / m : 1;
  if (by_points < k) k = by_points;
  if (n < k) k = n;
  return k < 1 ? 1 : k;
}

// The plan of a call: n sums of m terms (1 <= m <= BSUM_MAX_TERMS) in `passes` passes of sums_per_pass sums, the last of
// last_sums; `full` is msm_plan for a pass of sums_per_pass sums and `last` that of the last pass (equal when the passes are);
// the passes run back to back in one workspace of `bytes`, the larger of the two.
struct BsumPlanIn { size_t n, m; int window_bits, cus, span_blocks; };
struct BsumPlan {
  int c;
  size_t sums_per_pass, passes, last_sums;
  MsmPlan full, last;
  size_t bytes;
};
inline MsmPlan bsum_pass_plan(size_t sums, size_t m, int c, int cus, int span_blocks) {
  MsmPlanIn in;
  in.n = sums * m; in.c = c; in.cus = cus; in.span_blocks = span_blocks; in.sums = sums;
  return msm_plan(in);
}
inline BsumPlan bsum_plan(const BsumPlanIn& in) {
  BsumPlan p{};
  p.c = in.window_bits ? in.window_bits : bsum_window(in.m);
  const size_t n = in.n < 1 ? 1 : in.n;                          // (the plan of an empty call is that of one sum)
  p.sums_per_pass = bsum_sums_per_pass(n, in.m, p.c);
  p.passes = (n + p.sums_per_pass - 1) / p.sums_per_pass;
  p.last_sums = n - (p.passes - 1) * p.sums_per_pass;
  p.full = bsum_pass_plan(p.sums_per_pass, in.m, p.c, in.cus, in.span_blocks);
  p.last = p.last_sums == p.sums_per_pass ? p.full : bsum_pass_plan(p.last_sums, in.m, p.c, in.cus, in.span_blocks);
  p.bytes = p.full.bytes > p.last.bytes ? p.full.bytes : p.last.bytes;
  return p;
}

}  // namespace d377
