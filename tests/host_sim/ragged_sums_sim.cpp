// Test-only host build of d377_batch_ragged_msm (decaf377_amd/csrc/msm_ragged.inc): the plan of msm_ragged_plan.hpp and, over
// it, the walk of every pass as the device runs it -- the sum of a term by the shared lookup, tile by tile as k_rsum_keys does
// it (rsum_tile_sum), the signed digits of k / 2 mod r (msm_digit), the composite keys by the shared function (bsum_key) in
// the digit type the plan chooses, the buckets by plain accumulation with the host build of curve.hpp, a bucket's owner and
// weight by the shared decode, Horner over the windows, the final doubling and the encoding.  NOT part of the product:
// compiled by tests/test_ragged_sums_host.py with g++ -- as a library, and with -DRAGGED_SIM_MAIN as a stand-alone program
// over one fixed case for the sanitizers --, it exists only under tests/.  It includes sim.cpp (sim_init, the record helpers).
#include <cstdio>
#include <map>

#include "sim.cpp"
#include "msm_ragged_plan.hpp"

static ge rgs_small_mul(const ge& g, uint32_t s) {
  ge r = ge_identity();
  for (int bit = 31; bit >= 0; --bit) {
    r = ge_double(r);
    if ((s >> bit) & 1u) r = ge_add(r, g);
  }
  return r;
}

extern "C" {

uint32_t rgs_sum_of_term(const uint64_t* off, uint32_t K, uint64_t g) { return rsum_sum_of_term(off, K, g); }
uint32_t rgs_tile_sum(const uint64_t* off, uint32_t K, uint64_t base, size_t n, size_t i) { return rsum_tile_sum(off, K, base, n, i); }
int rgs_window(uint64_t terms, size_t n, int window_bits) { return rsum_window(terms, n, window_bits); }
size_t rgs_first_bad_sum(const uint64_t* off, size_t n) { return rsum_first_bad_sum(off, n); }
size_t rgs_device_cut(const uint64_t* off, size_t n, size_t devices, size_t k) { return rsum_device_cut(off, n, devices, k); }

// head = {c, passes, max_sums, max_points, bytes}
void rgs_plan(const uint64_t* off, size_t n, int window_bits, int cus, int span_blocks, int64_t* head) {
  const RsumPlan p = rsum_plan(off, n, window_bits, cus, span_blocks);
  head[0] = p.c; head[1] = (int64_t)p.passes; head[2] = (int64_t)p.max_sums; head[3] = (int64_t)p.max_points; head[4] = (int64_t)p.bytes;
}
// out: up to cap triples (first, sums, points) -> the number of passes
size_t rgs_passes(const uint64_t* off, size_t n, int c, uint64_t* out, size_t cap) {
  size_t count = 0;
  for (size_t first = 0; first < n; ++count) {
    const RsumPass ps = rsum_next_pass(off, n, first, c);
    if (count < cap) { out[3 * count] = ps.first; out[3 * count + 1] = ps.sums; out[3 * count + 2] = ps.points; }
    first += ps.sums;
  }
  return count;
}

// n sums delimited by off[0 .. n]: pts off[n] Element records (or, encoded != 0, Encodings), k off[n] scalars; enc_out n x 8
// words, xyzt_out n x 32 words (or null), status off[n] bytes (encoded only).  stats (or null): [0] passes walked, [1] the
// largest |key| stored, [2] 1 if any pass stored its keys as int32, [3] 1 if any as int16, [4] passes without a point.
int rgs_walk(int encoded, const uint32_t* pts, const uint32_t* k, const uint64_t* off, size_t n, int window_bits, int cus, uint32_t* enc_out,
             uint32_t* xyzt_out, uint8_t* status, int64_t* stats) {
  if (window_bits && (window_bits < BSUM_MIN_WINDOW || window_bits > BSUM_MAX_WINDOW)) return -1;
  if (n && (off[0] != 0 || rsum_first_bad_sum(off, n) < n)) return -1;
  const int c = rsum_window(n ? off[n] : 0, n, window_bits);
  int64_t st[5] = {0, 0, 0, 0, 0};
  for (size_t first = 0; first < n;) {
    const RsumPass ps = rsum_next_pass(off, n, first, c);
    const size_t K = ps.sums, N = ps.points;
    ++st[0];
    if (N == 0) {                                                 // k_rsum_empty
      ++st[4];
      for (size_t s = 0; s < K; ++s) {
        const ge r = ge_double(ge_identity());
        if (xyzt_out) ge_store256(r, xyzt_out + 32 * (first + s));
        RegPowTab pt;
        ge_compress(g_T, pt, r, enc_out + 8 * (first + s));
      }
      first += K;
      continue;
    }
    const MsmPlan p = rsum_pass_plan(ps, c, cus, 4);
    const WinShape ws = p.shape;
    const int W = ws.W, nb = p.nb;
    if (p.sums != K || (size_t)(nb - 1) != K << (c - 1)) return -2;
    st[p.wide_digits ? 2 : 3] = 1;
    const uint64_t* poff = off + first;                           // the pass's K + 1 offsets
    const uint64_t base = off[first];
    std::map<uint64_t, ge> bucket;                                // (w, j) -> the bucket's sum; absent = empty
    for (size_t i = 0; i < N; ++i) {                              // pass-local point i
      const size_t gi = (size_t)base + i;
      const uint32_t sum = rsum_tile_sum(poff, (uint32_t)K, base, N, i);
      if (sum >= K || !(poff[sum] <= gi && gi < poff[sum + 1])) return -6;
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
        int key = bsum_key(sum, c, d);
        key = p.wide_digits ? (int)(int32_t)key : (int)(int16_t)key;   // the digit type of the pass
        if (key == 0) continue;
        const int64_t a = key < 0 ? -(int64_t)key : key;
        if (a > st[1]) st[1] = a;
        if (a >= nb) return -3;
        const uint64_t slot = (uint64_t)w * (uint64_t)nb + (uint64_t)a;
        const ge term = key < 0 ? ge_neg(g) : g;
        auto it = bucket.find(slot);
        if (it == bucket.end()) bucket[slot] = term; else it->second = ge_add(it->second, term);
      }
      if (carry) return -4;
    }
    std::vector<ge> S((size_t)W * K, ge_identity());              // the weighted sums of the W K pseudo-windows
    for (const auto& e : bucket) {
      const int w = (int)(e.first / (uint64_t)nb);
      const uint32_t j = (uint32_t)(e.first % (uint64_t)nb);
      const uint32_t sum = bsum_bucket_sum(j, c), wt = bsum_bucket_weight(j, c);
      if (sum >= K || bsum_leaf_base(w, sum, nb, c) + wt != e.first) return -5;
      S[(size_t)w * K + sum] = ge_add(S[(size_t)w * K + sum], rgs_small_mul(e.second, wt));
    }
    for (size_t s = 0; s < K; ++s) {                              // k_bsum_final
      ge acc = S[(size_t)(W - 1) * K + s];
      for (int w = W - 2; w >= 0; --w) {
        for (int j = 0; j < ws.width(w); ++j) acc = ge_double(acc);
        acc = ge_add(acc, S[(size_t)w * K + s]);
      }
      const ge r = ge_double(acc);                                // the scalars were halved
      if (xyzt_out) ge_store256(r, xyzt_out + 32 * (first + s));
      RegPowTab pt;
      ge_compress(g_T, pt, r, enc_out + 8 * (first + s));
    }
    first += K;
  }
  if (stats) for (int i = 0; i < 5; ++i) stats[i] = st[i];
  return 0;
}

}

#ifdef RAGGED_SIM_MAIN
// One fixed case for the sanitizers: points j G, small scalars, lengths with empty sums at both ends and in the middle,
// several passes at the widest window; every sum against its double-and-add value, and the lookup on a hostile array.
int main() {
  sim_init();
  const size_t lengths[] = {0, 5, 0, 0, 300, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                            0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7, 0};
  const size_t n = sizeof lengths / sizeof lengths[0];
  std::vector<uint64_t> off(n + 1, 0);
  for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + lengths[i];
  const size_t terms = (size_t)off[n];
  uint32_t gen[32];
  {
    // the generator from its Encoding (8 followed by zeros)
    uint32_t enc[8] = {8, 0, 0, 0, 0, 0, 0, 0};
    RegPowTab pt;
    ge g;
    if (ge_decompress(g_T, pt, enc, &g) != 0) { printf("generator\n"); return 2; }
    ge_store256(g, gen);
  }
  const ge G = ge_load256(gen);
  std::vector<uint32_t> pts(32 * terms), k(8 * terms, 0), enc(8 * n, 0xA5A5A5A5u), el(32 * n);
  ge run = G;
  for (size_t j = 0; j < terms; ++j) {                            // point j = (j + 1) G, scalar 2 (3 j + 1): the walk halves it
    ge_store256(run, pts.data() + 32 * j);
    run = ge_add(run, G);
    k[8 * j] = (uint32_t)(2 * (3 * j + 1));
  }
  for (int wb : {16, 4, 0}) {
    int64_t stats[5];
    const int rc = rgs_walk(0, pts.data(), k.data(), off.data(), n, wb, 256, enc.data(), el.data(), nullptr, stats);
    if (rc) { printf("walk %d at window_bits %d\n", rc, wb); return 3; }
    for (size_t s = 0; s < n; ++s) {
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
      if (memcmp(we, enc.data() + 8 * s, 32) != 0) { printf("sum %zu differs at window_bits %d\n", s, wb); return 4; }
    }
    if (wb == 16 && (stats[0] < 3 || stats[4] < 1)) { printf("passes %lld, empty %lld\n", (long long)stats[0], (long long)stats[4]); return 5; }
  }
  const uint64_t hostile[6] = {~0ull, 3, 0, ~0ull, 1, 2};
  for (uint32_t K = 1; K <= 6; ++K)
    for (uint64_t g : {0ull, 1ull, 2ull, 3ull, 1000ull, ~0ull})
      if (rgs_sum_of_term(hostile, K, g) >= K || rgs_tile_sum(hostile, K, g, 700, 300) >= K) { printf("clamp\n"); return 6; }
  printf("RAGGED_SIM_OK\n");
  return 0;
}
#endif
