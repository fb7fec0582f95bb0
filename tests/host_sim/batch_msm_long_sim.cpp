// Test-only host build of d377_batch_msm_long (decaf377_amd/csrc/batch_msm_long.hip): the plan of batch_msm_long_plan.hpp,
// over it the lane kernel's walk -- every group one Straus chain of b slots (straus.hpp, the device's own), the slots of a sum's
// last group that lie past its end dead and reading nothing -- the partial sums written as Element records (the double of the
// chain's result), the fold levels with the records' own addition (ge_add_raw_words, what k_msm_long_fold runs), and the
// chunked compressor's pass with batched inversions on the last level's records.  NOT part of the product: compiled by
// tests/test_batch_msm_long_host.py with g++, it exists only under tests/.  It includes sim.cpp (sim_init, HostStrausTab,
// the record helpers).
#include "sim.cpp"
#include "batch_msm_long_plan.hpp"

extern "C" {

// the plan's numbers for the Python side: out = {g, b, first(q) and count(q) for q < g ...} (2 + 2 g words)
void bml_plan(size_t m, size_t* out) {
  const LongPlan p = long_plan(m);
  out[0] = p.g; out[1] = p.b;
  for (size_t q = 0; q < p.g; ++q) { out[2 + 2 * q] = p.first(q); out[3 + 2 * q] = p.count(q); }
}
int bml_fold() { return (int)BML_FOLD; }
// records per sum on every fold level from g down to 1 -> how many levels
int bml_levels(size_t g, size_t* per_level) {
  int n = 0;
  for (size_t c = g; c > 1; c = fold_out(c)) per_level[n++] = fold_out(c);
  return n;
}

// n sums of m > 8 terms: xyzt n x m Element records (or, encoded != 0, enc n x m Encodings), k n x m scalars; enc_out n x 8 words,
// xyzt_out n x 32 words (or null), status n x m bytes (encoded only).  touched (or null): n x m bytes, incremented for every
// term the point loader reads -- a dead slot must read nothing, so every term is read exactly once.
int bml_msm_long(int encoded, const uint32_t* pts, const uint32_t* k, size_t m, size_t n, uint32_t* enc_out, uint32_t* xyzt_out,
                 uint8_t* status, uint8_t* touched) {
  if (m <= BML_GROUP_MAX || m > 4096) return -1;
  const LongPlan plan = long_plan(m);
  const size_t np = n * plan.g;
  std::vector<uint32_t> partials(np * 32);
  for (size_t i = 0; i < np; ++i) {                              // k_msm_long_lane's element i
    HostStrausTab tab;
    const size_t s = i / plan.g, q = i % plan.g;
    const size_t first = s * plan.m + plan.first(q);
    const int live = (int)plan.count(q);
    const ge r = straus_sum(tab, (int)plan.b,
      [&](int p, uint32_t kk[8]) {
        if (p < live) { memcpy(kk, k + 8 * (first + p), 32); return; }
        for (int w = 0; w < 8; ++w) kk[w] = 0;
      },
      [&](int p, ge* g) -> bool {
        if (p >= live) { *g = ge_identity(); return true; }
        if (touched) ++touched[first + p];
        if (encoded) {
          RegPowTab pt;
          const uint32_t bad = ge_decompress(g_T, pt, pts + 8 * (first + p), g);
          status[first + p] = (uint8_t)bad;
          return bad != 0;
        }
        *g = ge_load256(pts + 32 * (first + p));
        return fe_is_zero(g->z);
      }, DCB_WANT_T);
    ge_store256(ge_double_fast(r, true), partials.data() + 32 * i);
  }
  // k_msm_long_fold, level by level
  std::vector<uint32_t> cur = partials, next;
  for (size_t c = plan.g; c > 1; c = fold_out(c)) {
    const size_t oc = fold_out(c);
    next.assign(n * oc * 32, 0);
    for (size_t L = 0; L < n * oc; ++L) {
      const size_t s = L / oc, f = L % oc, lo = s * c + f * BML_FOLD;
      const int cnt = (int)fold_count(c, f);
      uint32_t acc[32];
      memcpy(acc, cur.data() + 32 * lo, 128);
      for (int j = 1; j < cnt; ++j) {
        uint32_t r[32];
        ge_add_raw_words(acc, cur.data() + 32 * (lo + j), false, r);
        memcpy(acc, r, 128);
      }
      memcpy(next.data() + 32 * L, acc, 128);
    }
    cur.swap(next);
  }
  if (xyzt_out) memcpy(xyzt_out, cur.data(), n * 128);
  sim_compress_assisted(cur.data(), n, enc_out);                 // k_compress_chunked's rounds
  return 0;
}

}
