// Test-only host build of d377_batch_bucket_msm (decaf377_amd/csrc/msm_batch.inc): the plan of msm_batch_plan.hpp and, over it,
// the walk of every pass as the device runs it -- the signed digits of k / 2 mod r (msm_digit), the composite keys by the
// shared function (bsum_key), stored in the digit type the plan chooses, the buckets by plain accumulation with the host build
// of curve.hpp, a bucket's owner and weight by the shared decode, Horner over the windows with WinShape, the final doubling
// and the encoding.  NOT part of the product: compiled by tests/test_bucket_sums_host.py with g++, it exists only under
// tests/.  It includes sim.cpp (sim_init, the record helpers).
#include <map>

#include "sim.cpp"
#include "msm_batch_plan.hpp"

static ge small_mul(const ge& g, uint32_t s) {
  ge r = ge_identity();
  for (int bit = 31; bit >= 0; --bit) {
    r = ge_double(r);
    if ((s >> bit) & 1u) r = ge_add(r, g);
  }
  return r;
}

static void put_plan(const MsmPlan& p, int64_t* o, uint64_t* off, uint64_t* sz) {
  const int64_t v[] = {(int64_t)p.W, (int64_t)p.nb, (int64_t)p.sums, (int64_t)p.pw, p.wide_digits, p.packed, p.tree, (int64_t)p.ws_depth, (int64_t)p.ws_m,
                        (int64_t)p.ws_nblk, p.block_kernel == WSUM_BLOCK8, p.ws_mid, (int64_t)p.top_m, (int64_t)p.top_nblk, (int64_t)p.top_stride,
                        (int64_t)p.wsb_lds, (int64_t)p.count_parts, (int64_t)p.count_nbr, (int64_t)p.hist_bytes, (int64_t)p.bytes, (int64_t)p.shape.c,
                        (int64_t)p.scan_chunks, (int64_t)p.S, (int64_t)p.per, (int64_t)p.max_segs, (int64_t)p.span_lanes_max};
  for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) o[i] = v[i];
  for (int r = 0; r < R_COUNT; ++r) { off[r] = p.region[r].offset; sz[r] = p.region[r].bytes; }
}

extern "C" {

int bks_window(size_t m) { return bsum_window(m); }
int bks_key(uint32_t k, int c, int d) { return bsum_key(k, c, d); }
int bks_key_digit(int key, int c, uint32_t* k) { return bsum_key_digit(key, c, k); }
void bks_bucket_owner(uint32_t j, int c, uint32_t* sum, uint32_t* weight) { *sum = bsum_bucket_sum(j, c); *weight = bsum_bucket_weight(j, c); }
uint64_t bks_leaf_base(int w, uint64_t k, int nb, int c) { return bsum_leaf_base(w, (size_t)k, nb, c); }

// head = {c, sums_per_pass, passes, last_sums, bytes}; full / last: 26 decisions each (put_plan) and the R_COUNT regions;
// consts = {PT_WORDS, NODE_STRIDE, R_NODES, R_SUMS, R_BUCKETS, R_DIGITS, R_IDX, R_PTS, R_CHUNKS, R_FOLD0, R_FOLD1, R_MID}.  -> R_COUNT
int bks_plan(size_t n, size_t m, int window_bits, int cus, int span_blocks, int64_t* head, int64_t* full, uint64_t* off_full, uint64_t* sz_full,
             int64_t* last, uint64_t* off_last, uint64_t* sz_last, int* consts) {
  const BsumPlan p = bsum_plan(BsumPlanIn{n, m, window_bits, cus, span_blocks});
  head[0] = p.c; head[1] = (int64_t)p.sums_per_pass; head[2] = (int64_t)p.passes; head[3] = (int64_t)p.last_sums; head[4] = (int64_t)p.bytes;
  put_plan(p.full, full, off_full, sz_full);
  put_plan(p.last, last, off_last, sz_last);
  const int cs[] = {PT_WORDS, NODE_STRIDE, R_NODES, R_SUMS, R_BUCKETS, R_DIGITS, R_IDX, R_PTS, R_CHUNKS, R_FOLD0, R_FOLD1, R_MID};
  for (size_t i = 0; i < sizeof cs / sizeof cs[0]; ++i) consts[i] = cs[i];
  return R_COUNT;
}

// n sums of m terms: pts n x m Element records (or, encoded != 0, Encodings), k n x m scalars; enc_out n x 8 words, xyzt_out
// n x 32 words (or null), status n x m bytes (encoded only).  stats (or null): [0] passes walked, [1] the largest |key| stored,
// [2] 1 if any pass stored its keys as int32, [3] 1 if any as int16, [4] non-zero keys stored.
int bks_walk(int encoded, const uint32_t* pts, const uint32_t* k, size_t m, size_t n, int window_bits, int cus, uint32_t* enc_out,
             uint32_t* xyzt_out, uint8_t* status, int64_t* stats) {
  if (m < 1 || m > BSUM_MAX_TERMS || (window_bits && (window_bits < BSUM_MIN_WINDOW || window_bits > BSUM_MAX_WINDOW))) return -1;
  const BsumPlan bp = bsum_plan(BsumPlanIn{n, m, window_bits, cus, 4});
  int64_t st[5] = {0, 0, 0, 0, 0};
  for (size_t pass = 0; pass < (n ? bp.passes : 0); ++pass) {
    const size_t lo = pass * bp.sums_per_pass, K = pass + 1 < bp.passes ? bp.sums_per_pass : bp.last_sums;
    const MsmPlan& p = pass + 1 < bp.passes ? bp.full : bp.last;
    const WinShape ws = p.shape;
    const int c = ws.c, W = ws.W, nb = p.nb;
    if (p.sums != K || (size_t)(nb - 1) != K << (c - 1)) return -2;
    ++st[0];
    st[p.wide_digits ? 2 : 3] = 1;
    std::map<uint64_t, ge> bucket;                                // (w, j) -> the bucket's sum; absent = empty
    for (size_t i = 0; i < K * m; ++i) {                          // pass-local point i, sum i / m
      const size_t gi = lo * m + i;
      ge g;
      bool skip;
      if (encoded) {
        RegPowTab pt;
        const uint32_t bad = ge_decompress(g_T, pt, pts + 8 * gi, &g);
        status[gi] = (uint8_t)bad;
        skip = bad != 0;
      } else {
        g = ge_load256(pts + 32 * gi);
        skip = fe_is_zero(g.z);
      }
      uint32_t w8[8];
      for (int j = 0; j < 8; ++j) w8[j] = k[8 * gi + j];
      fr_reduce_words(w8);
      fr_half_words(w8);
      uint32_t carry = 0;
      for (int w = 0; w < W; ++w) {
        int d = msm_digit(w8, w, ws, carry);
        if (skip) d = 0;
        int key = bsum_key((uint32_t)(i / m), c, d);
        key = p.wide_digits ? (int)(int32_t)key : (int)(int16_t)key;   // the digit type of the pass
        if (key == 0) continue;
        const int64_t a = key < 0 ? -(int64_t)key : key;
        if (a > st[1]) st[1] = a;
        if (a >= nb) return -3;
        ++st[4];
        const uint64_t slot = (uint64_t)w * (uint64_t)nb + (uint64_t)a;
        const ge term = key < 0 ? ge_neg(g) : g;
        auto it = bucket.find(slot);
        if (it == bucket.end()) bucket[slot] = term; else it->second = ge_add(it->second, term);
      }
      if (carry) return -4;
    }
    // the weighted sums of the W K pseudo-windows, owner and weight by the shared decode
    std::vector<ge> S((size_t)W * K, ge_identity());
    for (const auto& e : bucket) {
      const int w = (int)(e.first / (uint64_t)nb);
      const uint32_t j = (uint32_t)(e.first % (uint64_t)nb);
      const uint32_t sum = bsum_bucket_sum(j, c), wt = bsum_bucket_weight(j, c);
      if (sum >= K || bsum_leaf_base(w, sum, nb, c) + wt != e.first) return -5;
      S[(size_t)w * K + sum] = ge_add(S[(size_t)w * K + sum], small_mul(e.second, wt));
    }
    for (size_t s = 0; s < K; ++s) {                             // k_bsum_final
      ge acc = S[(size_t)(W - 1) * K + s];
      for (int w = W - 2; w >= 0; --w) {
        for (int j = 0; j < ws.width(w); ++j) acc = ge_double(acc);
        acc = ge_add(acc, S[(size_t)w * K + s]);
      }
      const ge r = ge_double(acc);                                // the scalars were halved
      if (xyzt_out) ge_store256(r, xyzt_out + 32 * (lo + s));
      RegPowTab pt;
      ge_compress(g_T, pt, r, enc_out + 8 * (lo + s));
    }
  }
  if (stats) for (int i = 0; i < 5; ++i) stats[i] = st[i];
  return 0;
}

}
