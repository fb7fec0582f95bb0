// msm_plan.hpp -- the integer plan of the multi-scalar multiplication (msm.hip): how the 252 scalar bits are cut into
// windows, the signed digits of a scalar, where the span sums leave a bucket's partial sums, and the plan of one call of the
// bucket method (msm_plan: every route, launch shape and workspace region as a function of n, the window width and the
// device's size).  Plain integer code shared by the device kernels, the launcher and the host simulation (tests/host_sim),
// which checks it against big-integer arithmetic and against its own invariants (tests/test_msm_plan_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "curve.hpp"
#include "launch_plan.hpp"

namespace d377 {

// The windows of the 252 scalar bits: W = ceil(252 / c) of them, the first `nwide` c bits wide and the rest c - 1, so that they
// tile the 252 bits exactly whatever c is (c = 16: twelve 16-bit and four 15-bit windows; 14 and 12 tile by themselves).  A
// uniform width with a ragged top window -- 12 significant bits at c = 16 -- would pile n / 2^10 points on each of a few
// hundred buckets; here the top window is at most one bit narrower than the others, and because k / 2 mod r < r < 2^250.23 its
// UNSIGNED digits (the top window is not wrapped) stay below 2^(width - 1.77) + 1: inside the 2^(width-1) buckets of its width.
struct WinShape {
  int c, W, nwide;
  D377_HD int width(int w) const { return w < nwide ? c : c - 1; }
  D377_HD int first_bit(int w) const { return w * c - (w > nwide ? w - nwide : 0); }
};
// The same cut for any bit count B (d377_msm_short: B = 8 * scalar_bytes + 1, the extra bit being the room the unwrapped top
// window needs for the carry of the signed digits below it): W = ceil(B / c) windows of the NARROWEST width c' = ceil(B / W)
// with which W windows tile B, the first nwide of them c' bits and the rest c' - 1 (65 bits at c = 16: five 13-bit windows,
// where "c and c - 1" would have to drop 15 bits from 5 windows).  The shape carries c': buckets per window, the digit type
// and the tree's depth follow it.  For B = 252 and every c in 4 .. 18, c' = c: win_shape(c) below is what it always was
// (tests/test_msm_short_host.py pins that).
constexpr int FR_BITS = 252;
inline WinShape win_shape_bits(int B, int c) {
  const int W = (B + c - 1) / c;
  const int cn = (B + W - 1) / W;
  return WinShape{cn, W, W - (W * cn - B)};
}
inline WinShape win_shape(int c) { return win_shape_bits(FR_BITS, c); }
inline int short_scalar_bits(int scalar_bytes) { return 8 * scalar_bytes + 1; }
// signed digit w of k (< 2^252): |digit| <= 2^(width - 1); the top window is not wrapped
D377_HD int msm_digit(const uint32_t k[8], int w, const WinShape& ws, uint32_t& carry) {
  const int bit = ws.first_bit(w), cw = ws.width(w);
  const int wi = bit >> 5, sh = bit & 31;
  uint64_t v = k[wi];
  if (wi + 1 < 8) v |= (uint64_t)k[wi + 1] << 32;
  uint32_t d = (uint32_t)((v >> sh) & ((1u << cw) - 1u)) + carry;
  carry = 0;
  if (w + 1 < ws.W && d >= (1u << (cw - 1))) { carry = 1; return (int)d - (1 << cw); }
  return (int)d;
}

// THE SPANS (msm.hip, k_msm_spans): lane k of a window takes the sorted entries [k L, (k + 1) L) and leaves one partial per
// bucket its span touches.  A bucket that holds the entries [o, o + size) of its window is touched by the lanes o / L ...
// (o + size - 1) / L:
D377_HD uint32_t span_first_lane(uint32_t o, uint32_t L) { return o / L; }
D377_HD uint32_t span_partials(uint32_t o, uint32_t size, uint32_t L) { return size != 0 ? (o + size - 1) / L - o / L + 1 : 0u; }

// ---- the bucket method's constants (the kernels of msm.hip read them here) ------------------------------------------------
// Sizes of device_util.hpp and row_ops.hpp (device-only headers) that the plan needs; msm.hip pins them with static_asserts.
//                                         (PLAN_BLOCK, BLOCK: launch_plan.hpp)
constexpr int PLAN_AP_WORDS = 32;       // AP_WORDS: the affine cached point record
constexpr int PLAN_RQ_WORDS = 64;       // row::RQ_WORDS: one record of the Horner chain in the lane-spread form
constexpr int PT_WORDS = 48;            // one cached or extended point record: 4 * SLOT words, 192 B
constexpr int LP_WORDS = 4 * NL;        // one point in LDS, structure-of-arrays (k_msm_wsum_*)
constexpr int CHUNK = 8;                // buckets per lane in k_msm_chunks (short chains: this phase is latency-bound)
constexpr int FOLD = 4;                 // points per lane in k_msm_fold (a serial chain per lane: short chains, more levels)
// Partial sums per lane in the further reduction levels (k_msm_reduce), level 2, 3, 4, and `skip`: a level runs only if some
// bucket still has more than this many partials; fewer are summed by the lane (or pair of lanes) that finishes the bucket.
// With the span sums a bucket of random scalars is left with 1 + size / L partials -- one to three -- so no level runs; the
// levels are for runs that hold most of the points (many equal scalars: one bucket with thousands of partials), which each
// level cuts by its group size.  (Rounds 3-4, one lane per <= seg points of a bucket: 4-30 partials per bucket, skip and
// the segment length swept at 2^16 ... 2^22, everything within 2 %.)
struct RedSizes { int g[3]; uint32_t skip; };
constexpr RedSizes RED_DEFAULT = {{8, 8, 32}, 32};
constexpr int REDUCE_LEVELS = 4;
// lvlmax (zeroed by the host before the launch) receives, per reduction level l and WINDOW w, the largest number of
// level-(l+1) partials any bucket of that window has -- lvlmax[l * LVL_STRIDE + w] -- and per level the largest over all
// windows, lvlmax[REDUCE_LEVELS * LVL_STRIDE + l].  A level returns at once when no window needs it, and leaves the
// windows alone whose buckets are down to `skip` partials: the lane that finishes the bucket adds those (k_msm_buckets).
constexpr int LVL_STRIDE = 64;
constexpr int LVL_WORDS = REDUCE_LEVELS * LVL_STRIDE + REDUCE_LEVELS;
constexpr int SEG_BLOCKS_PER_CU = 4;             // workgroups of k_msm_spans per CU (128 VGPRs: tests/test_codegen.py)
constexpr uint32_t SPAN_MIN = 8;                 // entries per lane at least (a lane's locate + store are worth ~1 addition)
// the plan's scalars on the device: [0] L, [1] entries of all windows, [2] lanes of all windows
constexpr int META_WORDS = 4;
struct WinInfo { uint32_t len, lane0, ne0, lanes; };     // per window; entry [W] holds the totals in lane0 / ne0
constexpr int SUPER_BITS = 7, SUPER = 1 << SUPER_BITS;   // the sort's super-buckets: 128 consecutive buckets
// PACKED (batches of up to 2^24 points): the level-1 entry is ONE word -- sign, the 7 bits of the bucket within its
// super-bucket, 24 bits of point index -- instead of a word and a byte in two arrays (the byte stores came in runs of a few
// dozen bytes: 5 bytes written and 5 read per entry became 4 and 4).
constexpr size_t PACKED_MAX_POINTS = (size_t)1 << 24;
constexpr int WS_M = 8;                          // 2^WS_M buckets per workgroup of k_msm_wsum_block / block2
constexpr int WS_M8 = 9;                         // 2^WS_M8 per workgroup of k_msm_wsum_block8 (eight buckets per lane)
constexpr int NODE_STRIDE = WS_M8 + 1;           // points per block node in global memory (a node of depth m uses m + 1)
constexpr int MID_STRIDE = 16;                   // points per node of the middle level (depth <= 15)
constexpr int WSM_CAP = 96;                      // points per LDS buffer of k_msm_wsum_mid: 8 nodes of 11 points after the first level of a 16-to-1 merge
// The two point buffers of k_msm_wsum_window (dynamic LDS): the level that merges the block nodes leaves 2^(depth-m-1) nodes
// of m + 2 points, the next half as many of m + 3, and from there the levels shrink; the second buffer also carries the
// depth + 1 row records of the Horner chain.  Depth 13 (14-bit windows): 160 + 88 points, 35 KB; depth 15 (16-bit): 640 + 352, 140 KB.
inline int wsb_cap0(int depth, int m) { return depth > m ? (1 << (depth - m - 1)) * (m + 2) : m + 1; }
inline int wsb_cap1(int depth, int m) {
  int pts = depth > m + 1 ? (1 << (depth - m - 2)) * (m + 3) : 0;
  const int rec = ((depth + 1) * PLAN_RQ_WORDS + LP_WORDS - 1) / LP_WORDS;       // the Horner chain's records, in points
  return pts > rec ? pts : rec;
}

// THE RULE FOR L, the entries per span lane, from the E entries of all windows: one generation of the lanes the kernel keeps
// resident (lanes_target: a window's last lane is part full, so W lanes are spare), never fewer than SPAN_MIN entries; a
// developer's forced_L overrides both.  k_msm_scan2 applies it on the device, where E is known.
D377_HD uint32_t span_len(uint32_t E, uint32_t lanes_target, uint32_t forced_L) {
  uint32_t L = forced_L ? forced_L : (E + lanes_target - 1) / lanes_target;
  if (L < SPAN_MIN && !forced_L) L = SPAN_MIN;
  if (L < 1) L = 1;
  return L;
}

// ---- the plan of one call ---------------------------------------------------------------------------------------------------
// The workspace regions, in the order they lie.  R_PARTIALS is lent out: until k_msm_spans writes the span partials into it,
// it holds the level-1 index array of the sort (R_TMP_IDX, W * n words) -- one region, two views, as large as the larger.
enum MsmRegion {
  R_FLAG, R_PTS, R_DIGITS, R_BLOCKHIST, R_OFFS, R_SEGOFF, R_BSZ, R_TOT, R_TOT2, R_META, R_WINFO,
  R_PARTIALS, R_TMP_IDX = R_PARTIALS,
  R_IDX, R_SUB, R_BUCKETS, R_RED1, R_RED2, R_RED3, R_LVLMAX, R_CHUNKS, R_FOLD0, R_FOLD1, R_NODES, R_MID, R_SUMS, R_COUNT
};
static_assert(R_RED3 - R_RED1 + 2 == REDUCE_LEVELS, "one region per further reduction level");
struct MsmSpan { size_t offset, bytes; };
enum MsmBlockKernel { WSUM_BLOCK8, WSUM_BLOCK2, WSUM_BLOCK };   // k_msm_wsum_block8 / _block2 / _block
struct MsmFoldStep { int m_in, m_out, buf; };                  // k_msm_fold: m_in records per window -> m_out, into R_FOLD0 + buf
constexpr int MSM_MAX_FOLDS = 8;                               // 4^8 chunks: windows of up to 20 bits

constexpr long long PLAN_DEFAULT = -1;                         // an override that is not set: the built-in rule
struct MsmPlanIn {
  size_t n;
  int c, cus, span_blocks;               // window width (msm.hip: pick_window), CUs, workgroups of k_msm_spans a CU holds (occupancy query)
  // the developer overrides D377_TUNE_MSM_SLICES, _SEG, _RED, _SKIP, _CHUNKED_SUMS, _SORT_PACKED
  long long slices = PLAN_DEFAULT, seg = PLAN_DEFAULT, red = PLAN_DEFAULT, skip = PLAN_DEFAULT, chunked_sums = PLAN_DEFAULT, sort_packed = PLAN_DEFAULT;
  // SUMS that share the pipeline (msm_batch_plan.hpp): n points, n / sums per sum, under composite bucket keys -- sum k owns the
  // buckets k 2^(c-1) + 1 .. (k + 1) 2^(c-1) of every window.  One sum (the default) is d377_msm's plan, unchanged.
  size_t sums = 1;
  // scalar bits the windows tile: 252 (k / 2 mod r of any scalar), or short_scalar_bits() for d377_msm_short's 8- and 16-byte scalars
  int bits = FR_BITS;
};
struct MsmPlan {
  WinShape shape; int W, nb;             // the windows; bucket indices 0 .. sums * 2^(c-1)
  size_t sums; int pw;                   // sums that share the buckets; pseudo-windows W * sums: the tree's windows, 2^(c-1) leaves each
  int S; size_t per;                     // slices per window of the counting sort, points per slice
  bool wide_digits;                      // |digit| <= 2^(c-1): int16 up to 16-bit windows, int32 beyond
  int count_parts, count_nbr; size_t hist_bytes;     // the counting pass: parts per window, buckets per part, its LDS histogram
  int scan_chunks;                       // workgroups per window of k_msm_scan1/2/3 (1024 buckets each)
  uint32_t lanes_target, forced_L;       // span_len's arguments
  size_t span_lanes_max, max_segs;       // lanes of k_msm_spans at most; partial slots: one per lane and one per non-empty bucket
  RedSizes red; size_t max_g[REDUCE_LEVELS];         // the reduction levels: group sizes, records at most per level
  bool packed;                           // the sort's level-1 entries in one word
  int bucket_lanes;                      // lanes per bucket of k_msm_buckets: 1 or 2
  bool tree;                             // weighted bucket sums by the pairwise tree (else the chunked running sums)
  int ws_depth; MsmBlockKernel block_kernel; int ws_m, ws_nblk;   // the tree's block level: node depth, nodes per window
  bool ws_mid; int mid_m, mid_nblk;      // the middle level (trees deeper than 15)
  int top_m, top_nblk, top_stride, cap0, cap1; size_t wsb_lds;   // what k_msm_wsum_window merges; its two LDS buffers in points, their bytes
  int nchunks, nfolds; MsmFoldStep fold[MSM_MAX_FOLDS];   // the chunked sums: chunks per window and the folds down to one record
  size_t partials_bytes, tmp_idx_bytes;  // the two uses of R_PARTIALS
  MsmSpan region[R_COUNT]; size_t bytes; // the workspace: its regions and its size
};

inline MsmPlan msm_plan(const MsmPlanIn& in) {
  auto tuned = [](long long v, long long dflt) { return v >= 0 ? v : dflt; };
  MsmPlan p{};
  const size_t n = in.n;
  p.shape = win_shape_bits(in.bits, in.c);                     // W windows of c or c - 1 bits that tile the scalar bits
  const int c = p.shape.c;                                     // (in.c for the 252 bits of a full scalar; no wider for short ones)
  const int W = p.W = p.shape.W;
  const size_t K = p.sums = in.sums < 1 ? 1 : in.sums;         // (msm_batch_plan.hpp keeps K 2^(c-1) within the sort's 2^17)
  const int nb = p.nb = (int)(K << (c - 1)) + 1;
  const int PW = p.pw = W * (int)K;
  // slices per window of the counting sort: enough workgroups to cover the chip, never less than 8192 points each
  // (W * S <= the 2 workgroups of 1024 threads a CU holds: with one more slice per window, 18 x 29 = 522 workgroups on 512
  // places, the count and level-1 placement kernels ran a second generation for ten workgroups)
  int S = (int)tuned(in.slices, (long long)((size_t)2 * in.cus / (size_t)W));   // developer override (sweeps): 1 .. 4096
  if ((size_t)S > (n + 8191) / 8192) S = (int)((n + 8191) / 8192);
  if (S < 1) S = 1;
  p.S = S; p.per = (n + (size_t)S - 1) / (size_t)S;
  p.wide_digits = nb - 1 > (1 << 15);                          // one sum: c > 16
  // the counting pass keeps a histogram of at most 2^15 + 1 buckets in LDS (128 KiB): wider windows are counted in parts
  p.count_parts = (nb + (1 << 15)) / ((1 << 15) + 1);
  p.count_nbr = (nb + p.count_parts - 1) / p.count_parts;
  p.hist_bytes = (size_t)p.count_nbr * 4;
  p.scan_chunks = (nb + 1 + 1023) / 1024;
  // the span sums: lanes resident at once, less one per window; entries per lane when a developer forces them
  const size_t span_resident = (size_t)in.cus * in.span_blocks * PLAN_BLOCK;
  p.lanes_target = (uint32_t)(span_resident - (size_t)W);
  p.forced_L = (uint32_t)tuned(in.seg, 0);
  // lanes at most: a window of len entries takes ceil(len / L) lanes, all of them floor(E / L) + W at most, and span_len
  // gives L >= SPAN_MIN and L >= E / lanes_target (or the forced L), with E <= n W
  const size_t ents = (size_t)n * W;
  p.span_lanes_max = p.forced_L ? ents / p.forced_L + (size_t)W + 1
                                : (ents / SPAN_MIN + (size_t)W + 1 < span_resident ? ents / SPAN_MIN + (size_t)W + 1 : span_resident);
  p.max_segs = p.span_lanes_max + (size_t)W * nb + 1;
  p.partials_bytes = p.max_segs * PT_WORDS * 4;
  p.tmp_idx_bytes = (size_t)W * n * 4;
  // further levels of the bucket reduction: groups of partials, then groups of those (never more than this many); every
  // level is launched and decides on the device whether it has anything to do (k_msm_scan2, lvlmax)
  p.red = RED_DEFAULT;
  p.red.g[0] = (int)tuned(in.red, p.red.g[0]);                 // developer overrides (sweeps): 2 .. 64, 1 .. 64
  p.red.skip = (uint32_t)tuned(in.skip, p.red.skip);
  p.max_g[0] = p.max_segs;
  for (int l = 1; l < REDUCE_LEVELS; ++l) p.max_g[l] = p.max_g[l - 1] / (size_t)p.red.g[l - 1] + (size_t)W * nb;
  p.packed = n <= PACKED_MAX_POINTS && tuned(in.sort_packed, 1) != 0;
  {
    // partials a bucket is left with when the scalars are random: 1 + its run / the entries per span lane; up to four are
    // one lane's work.  The estimate is span_len at E = n W without its rounding up (the mean, not a lane count): rounded,
    // it would move the choice where run / L is close to 3 (13-bit windows on 256 CUs).
    const double run = (double)n / (double)(nb - 1);
    double Lest = p.forced_L ? (double)p.forced_L : (double)n * W / (double)p.lanes_target;
    if (!p.forced_L && Lest < (double)SPAN_MIN) Lest = (double)SPAN_MIN;
    p.bucket_lanes = 1.0 + run / Lest <= 4.0 ? 1 : 2;
  }
  // weighted bucket sums by the pairwise tree (every width); the chunked running sums remain as a developer override
  // (D377_TUNE_MSM_CHUNKED_SUMS), the tree's cross-check
  p.tree = tuned(in.chunked_sums, 0) == 0 || K > 1;           // (several sums: the tree alone knows pseudo-windows)
  // the tree's leaves are buckets 1 .. 2^(c-1) (bucket 0 is empty) of each sum: depth c - 1, a whole number of blocks
  const int depth = p.ws_depth = c - 1;
  // trees deeper than 15 (17- and 18-bit windows): a middle level merges the block nodes 8 or 16 to 1 (k_msm_wsum_mid), down
  // to 16 nodes per window for k_msm_wsum_window
  p.ws_mid = p.tree && depth > 15;
  p.mid_m = depth - 4; p.mid_nblk = 16;
  // 512 leaves per workgroup (k_msm_wsum_block8) where 256 per workgroup would not fit the chip at once: three of those per
  // CU.  And always under the middle level, whose LDS buffers (WSM_CAP) hold the first level of its 8- or 16-to-1 merge of
  // 9-deep nodes and not that of 8-deep ones.  The CU-count rule alone says the same below 1280 CUs (c = 17: W = 15 and
  // 15 * 2^8 > 3 * cus; c = 18: below 2390 CUs; an MI355X has 256), so the second clause changes nothing on today's devices.
  const bool ws8 = depth >= WS_M8 && ((size_t)PW * ((size_t)1 << (depth - WS_M)) > (size_t)in.cus * 3 || p.ws_mid);
  p.ws_m = ws8 ? WS_M8 : (depth < WS_M ? depth : WS_M);        // >= 2: window widths start at 4 here
  p.ws_nblk = 1 << (depth - p.ws_m);
  p.block_kernel = ws8 ? WSUM_BLOCK8
                       : ((size_t)2 * PW * p.ws_nblk <= (size_t)in.cus * 4 ? WSUM_BLOCK2 : WSUM_BLOCK);   // two waves per block while every wave keeps its own SIMD
  if (p.tree) {
    p.top_m = p.ws_mid ? p.mid_m : p.ws_m; p.top_nblk = p.ws_mid ? p.mid_nblk : p.ws_nblk; p.top_stride = p.ws_mid ? MID_STRIDE : NODE_STRIDE;
    p.cap0 = wsb_cap0(depth, p.top_m); p.cap1 = wsb_cap1(depth, p.top_m);
    p.wsb_lds = (size_t)(p.cap0 + p.cap1) * LP_WORDS * sizeof(uint32_t);
  }
  // the chunked sums: CHUNK buckets per lane, then folds of FOLD records down to one per window, alternating between two
  // buffers; the first fold's output is the largest a buffer sees, the second's the largest the other sees
  p.nchunks = (nb - 1 + CHUNK - 1) / CHUNK;
  const size_t m1 = (size_t)(p.nchunks + FOLD - 1) / FOLD, m2 = (m1 + FOLD - 1) / FOLD;
  for (int m = p.nchunks; m > 1 && p.nfolds < MSM_MAX_FOLDS; m = p.fold[p.nfolds++].m_out)
    p.fold[p.nfolds] = MsmFoldStep{m, (m + FOLD - 1) / FOLD, p.nfolds & 1};
  // the workspace, every region on a 256-byte boundary
  size_t bytes[R_COUNT];
  bytes[R_FLAG] = 256;
  bytes[R_PTS] = n * PLAN_AP_WORDS * 4;
  bytes[R_DIGITS] = (size_t)W * n * (p.wide_digits ? 4 : 2);
  bytes[R_BLOCKHIST] = (size_t)W * S * nb * 4;
  bytes[R_OFFS] = (size_t)W * (nb + 1) * 4;
  bytes[R_SEGOFF] = (size_t)REDUCE_LEVELS * W * (nb + 1) * 4;
  bytes[R_BSZ] = (size_t)W * (nb + 1) * 4;
  bytes[R_TOT] = (size_t)W * p.scan_chunks * 4;
  bytes[R_TOT2] = (size_t)W * p.scan_chunks * REDUCE_LEVELS * 4;
  bytes[R_META] = META_WORDS * sizeof(uint32_t);
  bytes[R_WINFO] = (size_t)(W + 1) * sizeof(WinInfo);
  bytes[R_PARTIALS] = p.partials_bytes > p.tmp_idx_bytes ? p.partials_bytes : p.tmp_idx_bytes;
  bytes[R_IDX] = (size_t)W * n * 4;
  bytes[R_SUB] = (size_t)W * n;                                // level-1 placement: bucket index within the super-bucket
  bytes[R_BUCKETS] = (size_t)W * nb * PT_WORDS * 4;
  for (int l = 1; l < REDUCE_LEVELS; ++l) bytes[R_RED1 + l - 1] = p.max_g[l] * PT_WORDS * 4;
  bytes[R_LVLMAX] = LVL_WORDS * sizeof(uint32_t);
  bytes[R_CHUNKS] = K > 1 ? 0 : (size_t)W * p.nchunks * PT_WORDS * 4;
  bytes[R_FOLD0] = K > 1 ? 0 : (size_t)W * m1 * PT_WORDS * 4;
  bytes[R_FOLD1] = K > 1 ? 0 : (size_t)W * m2 * PT_WORDS * 4;
  bytes[R_NODES] = p.tree ? (size_t)PW * p.ws_nblk * NODE_STRIDE * PT_WORDS * 4 : 0;
  bytes[R_MID] = p.ws_mid ? (size_t)W * p.mid_nblk * MID_STRIDE * PT_WORDS * 4 : 0;
  bytes[R_SUMS] = (size_t)PW * PT_WORDS * 4;
  size_t off = 0;
  for (int r = 0; r < R_COUNT; ++r) {
    p.region[r] = MsmSpan{off, bytes[r]};
    off = (off + bytes[r] + 255) / 256 * 256;
  }
  p.bytes = off;
  return p;
}

}  // namespace d377
