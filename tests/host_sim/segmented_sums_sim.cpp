// Test-only host build of d377_batch_segmented_msm (decaf377_amd/csrc/batch_msm_segmented.hip): the plan of
// msm_segmented_plan.hpp for the Python side, and over it the walk the device runs -- one Straus chain per LIVE slot of the
// chains' space (straus.hpp, the device's own; a dead slot reads nothing and writes nothing), the slot-indexed fold levels and
// the sum-indexed last level with the records' own addition (ge_add_raw_words), and the chunked compressor's pass on the n
// compact records.  Every record area is filled with a poison pattern first and every read of a record is counted against the
// writes: the walk fails if it reads a record nobody wrote.  NOT part of the product: compiled by
// tests/test_segmented_sums_host.py with g++, it exists only under tests/.  It includes sim.cpp (sim_init, HostStrausTab, the
// record helpers).  With -DSEGMENTED_SIM_MAIN it is a stand-alone program over one fixed case, for the sanitizers.
#include "sim.cpp"
#include "msm_segmented_plan.hpp"

extern "C" {

// out = {terms, chain_slots, chains, max_len, levels, bmax, records, advised_route, space[0 .. 4], base[0 .. 5]}: 19 words
void sgs_plan(const uint64_t* off, size_t n, uint64_t* out) {
  const SegPlan p = seg_plan(off, n);
  out[0] = p.terms; out[1] = p.chain_slots; out[2] = p.chains; out[3] = p.max_len; out[4] = (uint64_t)p.levels; out[5] = (uint64_t)p.bmax;
  out[6] = p.records; out[7] = (uint64_t)p.advised_route;
  for (int l = 0; l <= SEG_MAX_LEVELS; ++l) out[8 + l] = p.space[l];
  for (int l = 0; l <= SEG_MAX_LEVELS + 1; ++l) out[13 + l] = p.base[l];
}
uint64_t sgs_chains_below_mean() { return SEG_CHAINS_BELOW_MEAN; }
int sgs_max_levels() { return SEG_MAX_LEVELS; }
uint64_t sgs_start(const uint64_t* off, size_t i, int level) { return seg_start(off, i, level); }
size_t sgs_space(uint64_t T, size_t n, int level) { return seg_space(T, n, level); }
size_t sgs_records(uint64_t L, int level) { return seg_records(L, level); }
int sgs_levels(uint64_t max_len) { return seg_levels(max_len); }
size_t sgs_find(const uint64_t* off, size_t n, int level, uint64_t p) { return seg_find(off, n, level, p); }
// out = {live, sum, q, first, count, b}
void sgs_chain(const uint64_t* off, size_t n, uint64_t T, int bmax, uint64_t p, uint64_t* out) {
  const SegChain c = seg_chain(off, n, T, bmax, p);
  out[0] = c.live; out[1] = c.sum; out[2] = c.q; out[3] = c.first; out[4] = (uint64_t)c.count; out[5] = (uint64_t)c.b;
}
// out = {live, sum, lo, count}
void sgs_fold(const uint64_t* off, size_t n, int level, size_t S_in, uint64_t p, uint64_t* out) {
  const SegFold f = seg_fold(off, n, level, S_in, p);
  out[0] = f.live; out[1] = f.sum; out[2] = f.lo; out[3] = (uint64_t)f.count;
}
void sgs_last(const uint64_t* off, size_t i, int levels, size_t S_in, uint64_t* out) {
  const SegFold f = seg_last(off, i, levels, S_in);
  out[0] = f.live; out[1] = f.sum; out[2] = f.lo; out[3] = (uint64_t)f.count;
}

// n sums delimited by off (off[0] may be > 0: a device's slice; the buffers begin at term off[0]): pts Element records (or,
// encoded != 0, Encodings), k scalars; enc_out n x 8 words, xyzt_out n x 32 words (or null), status one byte per term (encoded
// only).  touched: one byte per term, incremented for every term the point loader reads.  stats = {live chains, dead slots,
// slot-indexed levels, fold lanes that added, reads of a record nobody wrote}.  -> 0, or -1 when an unwritten record was read.
int sgs_walk(int encoded, const uint32_t* pts, const uint32_t* k, const uint64_t* off, size_t n, uint32_t* enc_out, uint32_t* xyzt_out,
             uint8_t* status, uint8_t* touched, int64_t* stats) {
  for (int j = 0; j < 5; ++j) stats[j] = 0;
  if (n == 0) return 0;
  const SegPlan sp = seg_plan(off, n);
  std::vector<uint32_t> area(sp.records * 32, 0xDEADBEEFu);
  std::vector<uint8_t> written(sp.records, 0);
  // k_seg_lane / k_seg_wave: slot p of level 0
  for (size_t p = 0; p < sp.chain_slots && sp.terms; ++p) {
    const SegChain c = seg_chain(off, n, sp.terms, sp.bmax, p);
    if (!c.live) { ++stats[1]; continue; }
    ++stats[0];
    HostStrausTab tab;
    const size_t first = (size_t)c.first;
    const int live = c.count;
    const ge r = straus_sum(tab, c.b,
      [&](int q, uint32_t kk[8]) {
        if (q < live) { memcpy(kk, k + 8 * (first + q), 32); return; }
        for (int w = 0; w < 8; ++w) kk[w] = 0;
      },
      [&](int q, ge* g) -> bool {
        if (q >= live) { *g = ge_identity(); return true; }
        if (touched) ++touched[first + q];
        if (encoded) {
          RegPowTab pt;
          const uint32_t bad = ge_decompress(g_T, pt, pts + 8 * (first + q), g);
          status[first + q] = (uint8_t)bad;
          return bad != 0;
        }
        *g = ge_load256(pts + 32 * (first + q));
        return fe_is_zero(g->z);
      }, DCB_WANT_T);
    ge_store256(ge_double_fast(r, true), area.data() + 32 * (sp.base[0] + p));
    written[sp.base[0] + p] = 1;
  }
  auto add_records = [&](size_t in_base, size_t lo, int cnt, uint32_t* out) {
    uint32_t acc[32];
    for (int j = 0; j < cnt; ++j) stats[4] += !written[in_base + lo + j];
    memcpy(acc, area.data() + 32 * (in_base + lo), 128);
    for (int j = 1; j < cnt; ++j) {
      uint32_t r[32];
      ge_add_raw_words(acc, area.data() + 32 * (in_base + lo + j), false, r);
      memcpy(acc, r, 128);
    }
    memcpy(out, acc, 128);
  };
  // k_seg_fold, level by level
  for (int l = 0; l < sp.levels; ++l) {
    ++stats[2];
    for (size_t p = 0; p < sp.space[l + 1]; ++p) {
      const SegFold f = seg_fold(off, n, l, sp.space[l], p);
      if (!f.live) continue;
      ++stats[3];
      add_records(sp.base[l], (size_t)f.lo, f.count, area.data() + 32 * (sp.base[l + 1] + p));
      written[sp.base[l + 1] + p] = 1;
    }
  }
  // k_seg_last
  uint32_t* sums = area.data() + 32 * sp.base[sp.levels + 1];
  for (size_t i = 0; i < n; ++i) {
    const SegFold f = seg_last(off, i, sp.levels, sp.space[sp.levels]);
    if (f.live) add_records(sp.base[sp.levels], (size_t)f.lo, f.count, sums + 32 * i);
    else ge_store256(ge_identity(), sums + 32 * i);
  }
  if (xyzt_out) memcpy(xyzt_out, sums, n * 128);
  sim_compress_assisted(sums, n, enc_out);                       // k_compress_chunked's rounds
  return stats[4] ? -1 : 0;
}

}

#ifdef SEGMENTED_SIM_MAIN
// One fixed case under the sanitizers: lengths with empty sums at both ends and in a run, a sum that needs a slot-indexed level,
// the walk twice (the whole call, and a slice whose first offset is not 0), every term read exactly once; then offsets that
// are not monotone, through every lookup.
#include <stdio.h>
int main() {
  sim_init();
  const uint64_t lengths[] = {0, 1, 7, 8, 9, 17, 0, 0, 15, 1, 0, 137, 3, 0};
  const size_t n = sizeof lengths / sizeof lengths[0];
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + lengths[i];
  const size_t terms = (size_t)off[n];
  uint32_t gen[32];
  {
    uint32_t enc[8] = {8, 0, 0, 0, 0, 0, 0, 0};                  // the generator from its Encoding (8 followed by zeros)
    RegPowTab pt;
    ge g;
    if (ge_decompress(g_T, pt, enc, &g) != 0) { printf("generator\n"); return 2; }
    ge_store256(g, gen);
  }
  const ge G = ge_load256(gen);
  std::vector<uint32_t> pts(32 * terms), k(8 * terms, 0);
  ge run = G;
  for (size_t j = 0; j < terms; ++j) {                            // point j = (j + 1) G, scalar 2 (3 j + 1): the walk halves it
    ge_store256(run, pts.data() + 32 * j);
    run = ge_add(run, G);
    k[8 * j] = (uint32_t)(2 * (3 * j + 1));
  }
  for (int pass = 0; pass < 2; ++pass) {
    const size_t lo = pass ? 3 : 0, cnt = n - lo;               // the slice begins at sum 3 (offset 8)
    const size_t t0 = (size_t)off[lo], tn = terms - t0;
    std::vector<uint32_t> enc(cnt * 8, 0xA5A5A5A5u), el(cnt * 32);
    std::vector<uint8_t> touched(tn, 0);
    int64_t stats[5];
    if (sgs_walk(0, pts.data() + 32 * t0, k.data() + 8 * t0, off.data() + lo, cnt, enc.data(), el.data(), nullptr, touched.data(), stats) != 0) {
      printf("walk read an unwritten record\n");
      return 3;
    }
    for (size_t j = 0; j < tn; ++j)
      if (touched[j] != 1) { printf("term %zu read %d times\n", j, (int)touched[j]); return 4; }
    if (stats[2] != 1) { printf("levels %lld\n", (long long)stats[2]); return 5; }
    for (size_t s = lo; s < n; ++s) {
      uint64_t mult = 0;                                          // sum s = mult G
      for (uint64_t j = off[s]; j < off[s + 1]; ++j) mult += (j + 1) * 2 * (3 * j + 1);
      ge want = ge_identity();
      for (int bit = 63; bit >= 0; --bit) {
        want = ge_double(want);
        if ((mult >> bit) & 1u) want = ge_add(want, G);
      }
      uint32_t we[8];
      RegPowTab pt;
      ge_compress(g_T, pt, want, we);
      if (memcmp(we, enc.data() + 8 * (s - lo), 32) != 0) { printf("sum %zu differs in pass %d\n", s, pass); return 6; }
    }
  }
  const uint64_t junk[][6] = {{~0ull, 3, 0, ~0ull, 1, 2}, {9, 8, 7, 6, 5, 4}, {0, 0, 0, 0, 0, 0}, {5, 1ull << 40, 5, 0, 1ull << 63, 5}};
  for (const auto& a : junk)
    for (int level = 0; level <= SEG_MAX_LEVELS; ++level)
      for (uint64_t p : {0ull, 1ull, 7ull, 600ull, ~0ull}) {
        if (seg_find(a, 5, level, p) >= 5) { printf("find out of range\n"); return 1; }
        const SegChain c = seg_chain(a, 5, 40, 8, p);
        if (c.live && (c.first + (uint64_t)c.count > 40 || c.count < 1 || c.b > 8 || c.count > c.b)) { printf("chain out of range\n"); return 1; }
        if (level < SEG_MAX_LEVELS) {
          const SegFold f = seg_fold(a, 5, level, 11, p);
          if (f.live && (f.lo + (uint64_t)f.count > 11 || f.count < 1 || f.count > 16)) { printf("fold out of range\n"); return 1; }
        }
        for (size_t i = 0; i < 5; ++i) {
          const SegFold f = seg_last(a, i, level, 11);
          if (f.live && (f.lo + (uint64_t)f.count > 11 || f.count > 16)) { printf("last out of range\n"); return 1; }
        }
      }
  printf("SEGMENTED_SIM_OK\n");
  return 0;
}
#endif
