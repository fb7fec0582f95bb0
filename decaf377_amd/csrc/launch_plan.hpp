// launch_plan.hpp -- the integer plan of a batch launch: which kernel family a call of the generic launcher (d377.hip:
// launch) takes, its grid and block, whether it holds the lane-set guard, and how a chunked kernel's rounds are dealt out to
// its workgroups -- for the launcher's ops and for the batched sums (batch_host.hpp: lane_chunks; the sums' wave-or-lane
// rule).  A function of (op, n, CUs, tuning) and nothing else: plain integer code without the HIP runtime, shared by the
// launchers and the host simulation (tests/host_sim), which checks it against a record of the launcher it was lifted from
// and against its own invariants (tests/test_launch_plan_host.py).  Written like msm_plan.hpp, the MSM's plan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/decaf377_amd.h"

namespace d377 {

// Developer tuning (d377_ctx_set_tuning): one value per D377_TUNE_* key, D377_TUNE_DEFAULT = the built-in rule.  Lives in
// the context, written and read under d377_ctx::mu (every launch path holds it); nothing on a call path reads the
// process environment.
struct Tuning {
  int64_t v[D377_TUNE_COUNT];
  Tuning() { for (int k = 0; k < D377_TUNE_COUNT; ++k) v[k] = D377_TUNE_DEFAULT; }
};

// Constants of device-only headers that the plan needs; the units that own them pin each with a static_assert.
constexpr int PLAN_BLOCK = 256;                   // BLOCK (device_util.hpp)
#ifndef D377_WAVES_PER_SIMD
#define D377_WAVES_PER_SIMD 2
#endif
constexpr int PLAN_WAVES_PER_SIMD = D377_WAVES_PER_SIMD;   // WAVES_PER_SIMD (device_util.hpp)
#ifndef D377_DCB_K
#define D377_DCB_K 8
#endif
constexpr int PLAN_DCB_K = D377_DCB_K;            // DCB_K (curve.hpp)
constexpr int PLAN_DCB_KMAX = 16;                 // DCB_KMAX (dcb.hpp)
constexpr int PLAN_DCB_K_LONG = PLAN_DCB_KMAX;    // DCB_K_LONG (dcb.hpp)
#ifndef D377_FB_SETS
#define D377_FB_SETS 3
#endif
constexpr int PLAN_FB_SETS = D377_FB_SETS, PLAN_FB_K = 16;   // FB_SETS, FB_K (dcb.hpp)
constexpr int PLAN_FB_WIDE_GENERATIONS = 1;       // FB_WIDE_GENERATIONS (dcb.hpp)
constexpr int PLAN_SMALL_THREADS = 64, PLAN_SMALL_QUADS = PLAN_SMALL_THREADS / 4;   // SMALL_THREADS, SMALL_QUADS (d377.hip)
constexpr int PLAN_TINY4 = 4;                     // TINY4 (d377.hip)
constexpr int PLAN_CODEC_CHUNKED_MIN = 2;         // CODEC_CHUNKED_MIN (d377.hip)
constexpr int PLAN_AFFINE_PER_LANE = 32;          // AFFINE_PER_LANE (d377.hip)

// op codes of the generic launcher in d377.hip (shared with the sharded path)
enum Op { OP_SQRT, OP_DECOMPRESS, OP_COMPRESS, OP_ROUNDTRIP, OP_MUL_BASE, OP_MUL_VAR, OP_ENCODE, OP_HASH, OP_ADD, OP_DOUBLE,
          OP_EQ, OP_WIDE48, OP_WIDE64, OP_ENCODE_WIDE48, OP_ENCODE_WIDE64, OP_AFFINE, OP_NEG, OP_IS_IDENTITY, OP_FQ_BIN,
          OP_FQ_UN, OP_FQ_CHECKED, OP_FQ_TO_BYTES, OP_FR_MOD, OP_FR_CHECKED, OP_MUL_VAR_EL, OP_MUL_BASE_EL, OP_COMPRESS_FIELD,
          OP_ENCODE_EL, OP_HASH_EL, OP_FR_BIN, OP_FR_UN, OP_FR_WIDE48, OP_FR_WIDE64 };

// The device as the rules read it: its CU count and the owning context's overrides (null: none).  DeviceState derives from it.
struct PlanDev {
  int cus = 0;
  const Tuning* tune = nullptr;          // the owning context's overrides
  // the override for `key`, or `dflt` when the built-in rule is in force
  long long tuned(int key, long long dflt) const { return (tune && tune->v[key] >= 0) ? tune->v[key] : dflt; }
  bool is_tuned(int key) const { return tune && tune->v[key] >= 0; }
  // lanes the chunked kernels keep resident (WAVES_PER_SIMD workgroups of BLOCK lanes per CU): the unit the batch-size
  // thresholds of the launch rules are written in, so that they follow the device's CU count
  size_t resident_lanes() const { return (size_t)cus * PLAN_WAVES_PER_SIMD * PLAN_BLOCK; }
};

// At most cus * k workgroups of BLOCK lanes for `lanes` lanes (at least one): beyond, the kernel grid-strides.
inline int capped_grid(const PlanDev& d, size_t lanes, int k) {
  size_t blocks = (lanes + PLAN_BLOCK - 1) / PLAN_BLOCK;
  size_t cap = (size_t)d.cus * (size_t)k;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}
// Workgroups of BLOCK lanes for n elements: >> 256 workgroups when the batch allows it; capped so huge batches grid-stride
inline int grid_of(const PlanDev& d, size_t n) { return capped_grid(d, n, 32); }
// ... and the short kernels around the sums -- the fold levels of the long sums, the fixed-base segments, the index verdict
inline int fold_grid(const PlanDev& d, size_t lanes) { return capped_grid(d, lanes, 8); }

// How a chunked kernel's rounds (of BLOCK elements) are dealt out to its workgroups.  `places` workgroups are resident at a
// time and a chunk holds at most kmax rounds (elements per lane).  Up to one round per place: a workgroup per round.
// Otherwise G = the fewest generations of resident workgroups that can hold the rounds: exactly G x places chunks, the rounds
// dealt out evenly, the first `extra` chunks one round longer (DcbScratch::extra) -- every generation is full and there is
// no last generation of a few stragglers.  (Chunks of kmax left 5 x 2^18 elements with 128 of them: sqrt_ratio_zeta 2.54 ms
// against 2.13 dealt evenly, variable base 24.1 against 19.4: profiles/r05_chunk_between_generations.txt.)  Whole multiples
// of places x kmax rounds -- 2^20, 2^21, 2^22 elements on 256 CUs -- come out as chunks of kmax, as before.  Beyond `cap`
// chunks the workgroups walk several chunks of kmax.
struct ChunkDeal { size_t per_lane, extra, nchunks; };
inline ChunkDeal deal_chunks(size_t rounds, size_t places, size_t kmax, size_t cap) {
  ChunkDeal c{1, 0, rounds};
  if (rounds <= places) return c;
  const size_t gens = (rounds + places * kmax - 1) / (places * kmax);
  if (gens * places <= cap) {
    c.nchunks = gens * places; c.per_lane = rounds / c.nchunks; c.extra = rounds % c.nchunks;
  } else {
    c.per_lane = kmax; c.nchunks = (rounds + kmax - 1) / kmax;
    if (c.nchunks > cap) c.nchunks = cap;
  }
  return c;
}

// The chunks of a lane-set kernel over `count` elements: the launch's grid (one workgroup per chunk, oversubscribed on
// purpose, see DcbScratch) and the numbers of its DcbScratch.
// The batch in rounds of BLOCK elements over the `places` workgroups that are resident at once (cus x sets).  Up to
// kmax rounds per place everything runs in ONE generation, and the rounds are dealt out as evenly as they go: every
// workgroup takes rounds / places of them and the first rounds % places workgroups one more (DcbScratch::extra).
// (Chunks of ceil(n / resident lanes) elements per lane for everybody left a batch just above k x the resident lanes
// with fewer workgroups of k + 1 rounds each: pairs of them shared a CU while other CUs held one, and the call took
// as long as k + 1 full rounds -- profiles/r04_size_sweep.txt.)  Beyond that: the same deal over the fewest generations
// that hold the rounds (deal_chunks), as many workgroups as chunks.
// `tunable`: the generic launcher's form honours D377_TUNE_CHUNK_PER_LANE -- uniform chunks of that many rounds, at most kmax,
// their count capped as deal_chunks caps its own; the sums' form (lane_chunks) does not read the key.  Without the key the two
// forms are the same function.
struct LaneDeal { int grid, nslots, per_lane, extra, prio, kmax; };
inline LaneDeal lane_deal(const PlanDev& d, size_t count, int sets, int kmax, bool tunable) {
  const size_t places = (size_t)d.cus * (size_t)sets;
  const size_t rounds = (count + PLAN_BLOCK - 1) / PLAN_BLOCK;
  size_t per_lane, extra = 0, nchunks;
  if (tunable && d.is_tuned(D377_TUNE_CHUNK_PER_LANE)) {                    // developer override (sweeps, route tests): uniform chunks
    per_lane = (size_t)d.tuned(D377_TUNE_CHUNK_PER_LANE, 1);
    if (per_lane > (size_t)kmax) per_lane = (size_t)kmax;
    nchunks = (rounds + per_lane - 1) / per_lane;
    if (nchunks > (size_t)d.cus * 64) nchunks = (size_t)d.cus * 64;
  } else {
    const ChunkDeal c = deal_chunks(rounds, places, (size_t)kmax, (size_t)d.cus * 64);
    per_lane = c.per_lane; extra = c.extra; nchunks = c.nchunks;
  }
  // Issue priority by progress (dcb.hpp dcb_progress_priority) for launches of one or two generations of workgroups: there the
  // workgroups of a CU would end one after the other (-4 to -8 % at 2^20, -1 to -3 % at 1.5 and 2 x 2^20).  Longer launches
  // refill their CUs and only their last generation has that tail: within +-1 % either way at 2^22, so they stay as they
  // were measured (profiles/r05_ab_progress_priority.txt).
  return LaneDeal{(int)nchunks, d.cus * sets, (int)per_lane, (int)extra, nchunks <= 2 * places ? 1 : 0, kmax};
}

// Batches up to this many elements take the quad-per-element kernel (k_scalar_mul_var_small).  One wave of 16 quads per
// SIMD is 16 x 4 x CUs elements (16 384); the kernel still wins a little beyond that: the Element form (20 KiB of LDS per
// wave: seven waves per CU) runs 28 672 elements in one generation, two waves sharing most SIMDs -- 0.60 ms against 0.88
// with one lane per element -- and the Encoding form (39 KiB: four waves per CU) two generations of 16 384 in 1.02 ms
// against 1.08.  Beyond those sizes one lane per element is the better use of the chip (measured, profiles/README.md).
// D377_TUNE_SMALL_MAX: developer override (0 switches the small-batch kernel off).
inline size_t small_batch_max(const PlanDev& d, bool element_form) {
  return (size_t)d.tuned(D377_TUNE_SMALL_MAX, (long long)d.cus * PLAN_SMALL_QUADS * (element_form ? 7 : 8));
}

// Batches up to this many elements take one WAVE per element (k_scalar_mul_var_tiny): one wave per SIMD.  Capped by
// small_batch_max, so that switching the small-batch kernels off switches this one off too.  D377_TUNE_TINY_MAX: developer override.
inline size_t tiny_batch_max(const PlanDev& d) {
  const size_t v = (size_t)d.tuned(D377_TUNE_TINY_MAX, (long long)d.cus * 4), cap = small_batch_max(d, true);
  return v < cap ? v : cap;
}
// The batched sums' wave-or-lane rule (batch_msm.hip, batch_msm_long.hip and batch_msm_long_indexed.hip, by their sums or
// partial sums): up to four sums per SIMD a wave per sum (the lane kernel needs two sums per lane of the chip before it is the
// better use of it: 2^12 three-term sums 1.41 ms on lanes).  D377_TUNE_TINY_MAX, the developer override of every
// wave-per-element route, scales this one too.  Unlike tiny_batch_max it is not capped by small_batch_max: kept as measured.
inline size_t sums_wave_max(const PlanDev& d) { return 4 * (size_t)d.tuned(D377_TUNE_TINY_MAX, (long long)d.cus * 4); }

// ... and the square-root family's batches of up to FOUR elements per wave (d377.hip: k_*_tiny)
inline size_t tiny4_batch_max(const PlanDev& d) { return tiny_batch_max(d) * PLAN_TINY4; }
inline unsigned tiny4_grid(size_t n) { return (unsigned)((n + PLAN_TINY4 - 1) / PLAN_TINY4); }

// From this many elements decompress, compress and round trip run in chunks with batched inversions.
// from DCB_ASSIST_MIN elements per resident lane: the batched-inverse form (2^19 0.97 against 1.02 ms, 2^20 1.89 / 2.04,
// 2^21 3.79 / 4.06, 2^22 7.66 / 8.10); below, the wide grid
inline size_t codec_chunked_min(const PlanDev& d) {
  return (size_t)d.tuned(D377_TUNE_DECOMPRESS_CHUNKED_MIN, (long long)(d.resident_lanes() * PLAN_CODEC_CHUNKED_MIN));
}

// Large batches of the host-pointer path are pipelined in chunks of 2^18 records: while chunk k runs on the compute stream,
// chunk k+1's inputs are copied in and chunk k-1's outputs are copied out on the copy stream
// (double-buffered staging), so PCIe time hides under the kernels.
constexpr size_t PIPE_CHUNK = (size_t)1 << 18;
inline bool host_path_pipelined(size_t n) { return n >= 2 * PIPE_CHUNK; }

// ---- the plan of one call of the generic launcher ---------------------------------------------------------------------------
// The kernel family a call takes.  The launcher switches on (op, route) to the launch line.
enum Route {
  ROUTE_FOUR_PER_WAVE,       // four elements per wave: power chains on the rows, no scratch (k_*_tiny)
  ROUTE_PAIR_PER_WAVE,       // hash_to_curve, two pairs per wave: one pass over the rows for both maps (k_hash_to_curve_tiny2)
  ROUTE_WAVE_PER_ELEMENT,    // one element (scalar, sum) per wave, lane-spread arithmetic
  ROUTE_QUAD_PER_ELEMENT,    // one element per quad of lanes, table in LDS: no scratch, no hand-over
  ROUTE_LANE_SETS,           // one lane per element in chunks, each workgroup claiming a lane set of the scratch areas (dcb.hpp)
  ROUTE_CODEC_CHUNKED,       // ... the same by the kernels of codec_chunked.hip, if their residency allows it (the launcher asks
                             // codec_chunked_ok -- device state, not arithmetic -- and takes wide_grid_plan when it says no)
  ROUTE_WIDE_GRID,           // decompress / compress / round trip below codec_chunked_min: inversion-free, grid_of
  ROUTE_FB_NARROW,           // fixed base: WAVES_PER_SIMD workgroups per CU, DCB_K per inversion
  ROUTE_FB_WIDE,             // fixed base: FB_SETS workgroups per CU, FB_K per inversion
  ROUTE_EL_UNIFORM,          // k_scalar_mul_var_el: uniform chunks of one or two elements per lane
  ROUTE_AFFINE,              // k_to_affine: ~AFFINE_PER_LANE elements per lane
  ROUTE_PLAIN                // element-wise kernels: grid_of
};
struct LaunchPlan {
  Route route;
  int grid, block;
  bool guard;                // the launch acquires the lane-set guard (GuardScope on DeviceState::vb_guard)
  LaneDeal deal;             // routes that walk chunks (LANE_SETS, CODEC_CHUNKED, FB_*, EL_UNIFORM): the DcbScratch numbers; else zero
};
inline LaunchPlan plain_plan(Route r, int grid, int block) { return LaunchPlan{r, grid, block, false, LaneDeal{0, 0, 0, 0, 0, 0}}; }
inline LaunchPlan wide_grid_plan(const PlanDev& d, size_t n) { return plain_plan(ROUTE_WIDE_GRID, grid_of(d, n), PLAN_BLOCK); }
inline LaunchPlan dealt_plan(Route r, const LaneDeal& deal) { return LaunchPlan{r, deal.grid, PLAN_BLOCK, true, deal}; }

// n >= 1.  aux: launch()'s (no rule reads it today).
inline LaunchPlan launch_plan(Op op, int aux, size_t n, const PlanDev& d) {
  (void)aux;
  auto four = [&] { return plain_plan(ROUTE_FOUR_PER_WAVE, (int)tiny4_grid(n), 64); };
  auto wave = [&] { return plain_plan(ROUTE_WAVE_PER_ELEMENT, (int)n, 64); };
  auto quad = [&] { return plain_plan(ROUTE_QUAD_PER_ELEMENT, (int)((n + PLAN_SMALL_QUADS - 1) / PLAN_SMALL_QUADS), PLAN_SMALL_THREADS); };
  // Every kernel with a square root or an encoding keeps per-lane state in scratch areas that exist once per device
  // (round records of the batched inversions, window tables): never more lanes than those areas have, and each
  // launch queues behind the areas' last user.
  // kernels that work in chunks of DCB_K x 256 elements: one workgroup per chunk (oversubscribed on purpose, see
  // DcbScratch), each claiming one of the vb_blocks resident lane sets of the per-device scratch areas
  // DCB_K elements per lane when the batch is large enough to fill the resident lane sets that way, fewer otherwise
  // every chunked kernel but the fixed-base one (up to 2^20 on 256 CUs: <= DCB_K per lane either way)
  auto lanes = [&](Route r) { return dealt_plan(r, lane_deal(d, n, PLAN_WAVES_PER_SIMD, PLAN_DCB_K_LONG, true)); };
  switch (op) {
    case OP_SQRT:
    case OP_ENCODE:
      return n <= tiny4_batch_max(d) ? four() : lanes(ROUTE_LANE_SETS);
    case OP_DECOMPRESS:
      if (n <= tiny4_batch_max(d)) return four();
      return n >= codec_chunked_min(d) ? lanes(ROUTE_LANE_SETS) : wide_grid_plan(d, n);
    case OP_COMPRESS:
    case OP_ROUNDTRIP:
      if (n <= tiny4_batch_max(d)) return four();
      return n >= codec_chunked_min(d) ? lanes(ROUTE_CODEC_CHUNKED) : wide_grid_plan(d, n);   // as OP_DECOMPRESS
    case OP_HASH:
      if (n <= tiny4_batch_max(d) / 2) return plain_plan(ROUTE_PAIR_PER_WAVE, (int)((n + 1) / 2), 64);
      return n <= tiny4_batch_max(d) ? four() : lanes(ROUTE_LANE_SETS);
    case OP_MUL_BASE: {
      // Wide launch (3 workgroups per CU, 16 elements per inversion) beyond ONE generation of full narrow chunks (DCB_K elements per
      // resident lane: 2^20 on 256 CUs); up to there the narrow one (2 per CU, 8 per inversion), whose rounds are dealt out
      // evenly, is as fast or faster (196 608 elements: 166 against 186 us).  Beyond, the narrow launch needs a second
      // generation of workgroups and the wide one does not: wide / narrow 0.88 at 1.25 x 2^20, 0.95 at 1.5 x, 0.88 at
      // 1.75 x, 0.96 at 2^21, 0.94-0.95 at 3 x 2^20 and 2^22, warm clocks, alternating (profiles/r05_fb_wide_sweep.txt; the
      // threshold of rounds 3-4, two generations, was measured on the 18-bit comb before the rounds were dealt out evenly).
      if (n <= tiny_batch_max(d)) return wave();                // one scalar per wave, lane-spread arithmetic
      if (n <= small_batch_max(d, false)) return quad();        // one scalar per quad of lanes
      bool wide = n > d.resident_lanes() * PLAN_DCB_K * PLAN_FB_WIDE_GENERATIONS;
      if (d.is_tuned(D377_TUNE_FB_WIDE)) wide = d.tuned(D377_TUNE_FB_WIDE, 0) != 0;               // developer overrides (A/B)
      const int fk = (int)d.tuned(D377_TUNE_FB_K, wide ? PLAN_FB_K : PLAN_DCB_K);
      LaneDeal deal = lane_deal(d, n, wide ? PLAN_FB_SETS : PLAN_WAVES_PER_SIMD, fk, true);
      // dcb.hpp dcb_progress_priority in the wide launch: one generation only (-1 % at 1.25 x 2^20, -2 % at 2^21); two generations
      // of waves in step gather their table entries in bursts (+6 to +10 % at 2^22: profiles/r05_ab_progress_priority.txt)
      if (wide && deal.grid > d.cus * PLAN_FB_SETS) deal.prio = 0;
      return dealt_plan(wide ? ROUTE_FB_WIDE : ROUTE_FB_NARROW, deal);
    }
    case OP_MUL_VAR:
      if (n <= tiny_batch_max(d)) return wave();                // one element per wave, lane-spread arithmetic
      if (n <= small_batch_max(d, false)) return quad();        // one element per quad of lanes, table in LDS: no scratch, no hand-over
      return lanes(ROUTE_LANE_SETS);
    case OP_ENCODE_WIDE48:
    case OP_ENCODE_WIDE64:
    case OP_ENCODE_EL:
    case OP_HASH_EL:
      return lanes(ROUTE_LANE_SETS);
    case OP_AFFINE: {
      // ~AFFINE_PER_LANE elements per lane so that one inversion serves many, but never fewer lanes than one
      // wave per SIMD.  Measured (tools/attic/affine_bench.py, 2^20 elements): 0.28 / 0.40 / 0.65 / 1.14 ms at 1 / 2 / 4 / 8
      // blocks per CU -- every extra lane is an extra 380-operation inversion -- against 2.7 ms for one inversion
      // per element.  D377_TUNE_AFFINE_BLOCKS_PER_CU is a developer override for that sweep.
      size_t lanes_ = (n + PLAN_AFFINE_PER_LANE - 1) / PLAN_AFFINE_PER_LANE;
      const size_t fill = (size_t)d.cus * (size_t)d.tuned(D377_TUNE_AFFINE_BLOCKS_PER_CU, 1) * PLAN_BLOCK;
      if (lanes_ < fill) lanes_ = fill < n ? fill : n;
      return plain_plan(ROUTE_AFFINE, (int)((lanes_ + PLAN_BLOCK - 1) / PLAN_BLOCK), PLAN_BLOCK);
    }
    case OP_MUL_VAR_EL: {
      if (n <= tiny_batch_max(d)) return wave();
      if (n <= small_batch_max(d, true)) return quad();
      // no inversions here, so nothing argues for long chunks: one or two elements per lane keep the grid oversubscribed
      // at every batch size
      // (2^20 elements: 7.33e7/s with 8 per lane, 7.44 with 4, 7.59 with 2, 7.54 with 1)
      LaneDeal dv{0, d.cus * PLAN_WAVES_PER_SIMD, n > d.resident_lanes() ? 2 : 1, 0, 0, 2};   // this kernel walks uniform chunks
      size_t nch = (n + (size_t)dv.per_lane * PLAN_BLOCK - 1) / ((size_t)dv.per_lane * PLAN_BLOCK);
      if (nch > (size_t)d.cus * 64) nch = (size_t)d.cus * 64;
      dv.grid = (int)nch;
      // the lane-set deal carries the priority rule of ITS deal (chunks of up to 16 per lane); this launch has its own shape -- 8 192
      // chunks in 16 generations at 2^22 -- and the rule is about generations: priorities in launches of one or two of them
      dv.prio = nch <= 2 * (size_t)d.cus * PLAN_WAVES_PER_SIMD ? 1 : 0;
      return dealt_plan(ROUTE_EL_UNIFORM, dv);
    }
    case OP_MUL_BASE_EL:
      if (n <= tiny_batch_max(d)) return wave();
      if (n <= small_batch_max(d, true)) return quad();
      break;
    default:
      break;
  }
  return plain_plan(ROUTE_PLAIN, grid_of(d, n), PLAN_BLOCK);
}

}  // namespace d377
