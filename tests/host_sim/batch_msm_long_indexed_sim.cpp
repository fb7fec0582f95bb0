// Test-only host build of d377_batch_long_msm_indexed (decaf377_amd/csrc/batch_msm_long_indexed.hip): the cut of
// batch_msm_long_plan.hpp for any m of 1 .. 4096 (g = 1 for m <= 8), over it the lane kernel's walk -- every group one Straus
// chain of b slots (straus.hpp, the device's own), every slot classified by batch_msm_long_indexed_plan.hpp, the kernel's own
// function: live slots gather their record from the pool, slots past the end and absent or refused indices read nothing --
// the partial sums as Element records, the fold levels (none at g = 1, where the chains' records are the sums) and the chunked
// compressor's pass.  NOT part of the product: compiled by tests/test_msm_long_indexed_host.py with g++, it exists only under
// tests/.  It includes sim.cpp (sim_init, HostStrausTab, the record helpers).
#include "sim.cpp"
#include "batch_msm_long_indexed_plan.hpp"

extern "C" {

// the classification alone: kind[n x g x b] (0 past, 1 absent, 2 live) and record[n x g x b] for the Python side
void bmli_slots(size_t m, size_t n, const int* point_index, uint32_t pool_count, int* kind, long long* record) {
  const LongPlan plan = long_plan(m);
  size_t o = 0;
  for (size_t s = 0; s < n; ++s)
    for (size_t q = 0; q < plan.g; ++q)
      for (size_t p = 0; p < plan.b; ++p, ++o) {
        const LongSlot sl = long_indexed_slot(plan, s, q, (int)p, point_index, pool_count);
        kind[o] = sl.kind;
        record[o] = sl.kind == SLOT_LIVE ? (long long)sl.record : -1;
      }
}

// n sums of m terms: pool pool_count x 32 words, point_index n x m, k n x m scalars; enc_out n x 8 words, xyzt_out n x 32 words
// (or null).  pool_touched (or null): pool_count counters, one per record read; scalar_touched (or null): n x m counters, one per
// scalar read -- an absent term must read neither.
int bmli_msm(const uint32_t* pool, uint32_t pool_count, const int* point_index, const uint32_t* k, size_t m, size_t n, uint32_t* enc_out,
             uint32_t* xyzt_out, uint32_t* pool_touched, uint8_t* scalar_touched) {
  if (m < 1 || m > 4096 || pool_count < 1) return -1;
  const LongPlan plan = long_plan(m);
  const size_t np = n * plan.g;
  std::vector<uint32_t> partials(np * 32);
  for (size_t i = 0; i < np; ++i) {                              // k_msm_long_indexed_lane's element i
    HostStrausTab tab;
    const size_t s = i / plan.g, q = i % plan.g;
    const ge r = straus_sum(tab, (int)plan.b,
      [&](int p, uint32_t kk[8]) {
        const LongSlot sl = long_indexed_slot(plan, s, q, p, point_index, pool_count);
        if (sl.kind == SLOT_LIVE) {
          if (scalar_touched) ++scalar_touched[sl.term];
          memcpy(kk, k + 8 * sl.term, 32);
          return;
        }
        for (int w = 0; w < 8; ++w) kk[w] = 0;
      },
      [&](int p, ge* g) -> bool {
        const LongSlot sl = long_indexed_slot(plan, s, q, p, point_index, pool_count);
        if (sl.kind != SLOT_LIVE) { *g = ge_identity(); return true; }
        if (pool_touched) ++pool_touched[sl.record];
        *g = ge_load256(pool + 32 * sl.record);
        return fe_is_zero(g->z);
      }, DCB_WANT_T);
    ge_store256(ge_double_fast(r, true), partials.data() + 32 * i);
  }
  std::vector<uint32_t> cur = partials, next;
  for (size_t c = plan.g; c > 1; c = fold_out(c)) {              // k_msm_long_fold, level by level
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
