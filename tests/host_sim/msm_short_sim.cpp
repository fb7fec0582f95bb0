// Host build of msm_plan.hpp alone (test-only; never linked into the product) for d377_msm_short: the window shape for any bit
// count, the signed digits of 8- and 16-byte scalars exactly as msm.hip's msm_write_digits_short forms them (one zero-extended
// load, msm_digit per window: no reduction, no halving), and msm_plan with the bit count as an input.  Compiled by
// tests/test_msm_short_host.py with g++ as a shared library; with -DMSM_SHORT_SIM_MAIN it is a stand-alone program over fixed
// cases, for the sanitizers (-fsanitize=address,undefined, run as an ordinary program).
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "msm_plan.hpp"
using namespace d377;

namespace {
// win_shape(c) as it stood before the maker took a bit count, verbatim: what win_shape_bits(252, c) must equal
WinShape parent_win_shape(int c) {
  const int W = (252 + c - 1) / c;
  return WinShape{c, W, W - (W * c - 252)};
}
// the loader: `bytes` of the record, zero-extended to the eight words msm_digit reads
void short_words(const uint8_t* scalars, int bytes, size_t i, uint32_t k[8]) {
  for (int j = 0; j < 8; ++j) k[j] = 0;
  memcpy(k, scalars + i * (size_t)bytes, (size_t)bytes);     // (little-endian host, as the device)
}
}  // namespace

extern "C" {
// out = {c, W, nwide, first_bit(0 .. W-1) ..., width(0 .. W-1) ...}: 3 + 2 * 64 ints
void sim_short_shape(int B, int c, int* out) {
  const WinShape ws = win_shape_bits(B, c);
  out[0] = ws.c; out[1] = ws.W; out[2] = ws.nwide;
  for (int w = 0; w < ws.W && w < 64; ++w) { out[3 + w] = ws.first_bit(w); out[3 + 64 + w] = ws.width(w); }
}
void sim_parent_shape(int c, int* out) {
  const WinShape ws = parent_win_shape(c);
  out[0] = ws.c; out[1] = ws.W; out[2] = ws.nwide;
}
void sim_win_shape(int c, int* out) {                         // today's win_shape(c): the 252-bit case of the maker
  const WinShape ws = win_shape(c);
  out[0] = ws.c; out[1] = ws.W; out[2] = ws.nwide;
}
int sim_short_scalar_bits(int bytes) { return short_scalar_bits(bytes); }
// digits: n rows of 64 ints (W <= 63 used); [63] = the carry left after the top window, which must be 0
void sim_short_digits(const uint8_t* scalars, int bytes, size_t n, int c, int* digits) {
  const WinShape ws = win_shape_bits(short_scalar_bits(bytes), c);
  for (size_t i = 0; i < n; ++i) {
    uint32_t k[8], carry = 0;
    short_words(scalars, bytes, i, k);
    for (int w = 0; w < ws.W; ++w) digits[64 * i + w] = msm_digit(k, w, ws, carry);
    digits[64 * i + 63] = (int)carry;
  }
}
// msm_plan for in = {n, c, cus, span_blocks, slices, seg, red, skip, chunked_sums, sort_packed, bits}: the outputs and their order
// are those of sim.cpp's sim_msm_plan (tests/golden/msm_plan_parent.json's out_fields, then partials_bytes, tmp_idx_bytes,
// ws_depth, nfolds, then the width the shape carries), so that tests/test_msm_plan_host.py's Plan reads either.  -> R_COUNT.
int sim_msm_plan(const int64_t* in, int64_t* out, uint64_t* off, uint64_t* sz, int* fold, int* consts) {
  MsmPlanIn pi{};
  pi.n = (size_t)in[0]; pi.c = (int)in[1]; pi.cus = (int)in[2]; pi.span_blocks = (int)in[3];
  pi.slices = in[4]; pi.seg = in[5]; pi.red = in[6]; pi.skip = in[7]; pi.chunked_sums = in[8]; pi.sort_packed = in[9];
  pi.bits = (int)in[10];
  const MsmPlan p = msm_plan(pi);
  const int64_t v[] = {(int64_t)p.W, (int64_t)p.shape.nwide, (int64_t)p.nb, (int64_t)p.S, (int64_t)p.per, p.wide_digits, (int64_t)p.count_parts,
                        (int64_t)p.count_nbr, (int64_t)p.hist_bytes, (int64_t)p.scan_chunks, p.lanes_target, p.forced_L, (int64_t)p.span_lanes_max, (int64_t)p.max_segs,
                        (int64_t)p.red.g[0], (int64_t)p.red.g[1], (int64_t)p.red.g[2], p.red.skip, (int64_t)p.max_g[0], (int64_t)p.max_g[1], (int64_t)p.max_g[2],
                        (int64_t)p.max_g[3], p.packed, (int64_t)p.bucket_lanes, p.tree, p.block_kernel == WSUM_BLOCK8, (int64_t)p.block_kernel,
                        (int64_t)p.ws_m, (int64_t)p.ws_nblk, p.ws_mid, (int64_t)p.mid_m, (int64_t)p.mid_nblk, (int64_t)p.top_m,
                        (int64_t)p.top_nblk, (int64_t)p.top_stride, (int64_t)p.cap0, (int64_t)p.cap1, (int64_t)p.wsb_lds, (int64_t)p.nchunks, (int64_t)p.bytes,
                        (int64_t)p.partials_bytes, (int64_t)p.tmp_idx_bytes, (int64_t)p.ws_depth, (int64_t)p.nfolds};
  for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
  for (int r = 0; r < R_COUNT; ++r) { off[r] = p.region[r].offset; sz[r] = p.region[r].bytes; }
  for (int f = 0; f < p.nfolds; ++f) { fold[3 * f] = p.fold[f].m_in; fold[3 * f + 1] = p.fold[f].m_out; fold[3 * f + 2] = p.fold[f].buf; }
  const int cs[] = {PT_WORDS, FOLD, (int)SPAN_MIN, NODE_STRIDE, MID_STRIDE, WSM_CAP, R_PARTIALS, R_TMP_IDX, R_FOLD0, MSM_MAX_FOLDS, p.shape.c};
  for (size_t i = 0; i < sizeof cs / sizeof cs[0]; ++i) consts[i] = cs[i];
  return R_COUNT;
}
}  // extern "C"

#ifdef MSM_SHORT_SIM_MAIN
// Every export above over fixed cases: the shapes of every (B, c), the digits of the edge scalars and of seeded ones summed back
// modulo 2^128 (tests/test_msm_short_host.py does the exact sum with Python's integers), the plans of both lengths.
typedef unsigned __int128 u128;
static int check_digits(const uint8_t* rec, int bytes, int c) {
  int dg[64];
  sim_short_digits(rec, bytes, 1, c, dg);
  const WinShape ws = win_shape_bits(short_scalar_bits(bytes), c);
  u128 k = 0, sum = 0;
  memcpy(&k, rec, (size_t)bytes);
  for (int w = 0; w < ws.W; ++w) {
    const int lim = 1 << (ws.width(w) - 1);
    if (dg[w] > lim || dg[w] < -lim) return 1;
    const int bit = ws.first_bit(w);
    if (bit < 128) sum += (u128)(__int128)dg[w] << bit;        // (a window that starts at bit 128 holds the last carry: 0 mod 2^128)
  }
  if (dg[63] != 0) return 2;
  if (bytes == 8) { sum &= ((u128)1 << 64) - 1; }              // compared modulo 2^(8 bytes)
  return sum == k ? 0 : 3;
}
int main() {
  int shape[3 + 128], parent[3];
  for (int c = 4; c <= 18; ++c) {
    sim_short_shape(252, c, shape); sim_parent_shape(c, parent);
    if (shape[0] != parent[0] || shape[1] != parent[1] || shape[2] != parent[2]) { printf("shape 252 %d\n", c); return 1; }
  }
  uint64_t x = 0x9e3779b97f4a7c15ull;
  for (int bytes = 8; bytes <= 16; bytes += 8) {
    const int B = short_scalar_bits(bytes);
    for (int c = 4; c <= 16; ++c) {
      sim_short_shape(B, c, shape);
      const int W = shape[1];
      if (W > 63 || shape[3 + W - 1] + shape[3 + 64 + W - 1] != B) { printf("shape %d %d\n", B, c); return 1; }
      uint8_t rec[16];
      for (int e = 0; e < 4 + 256; ++e) {
        u128 k;
        if (e == 0) k = 0;
        else if (e == 1) k = 1;
        else if (e == 2) k = bytes == 16 ? ~(u128)0 : (u128)~0ull;
        else if (e == 3) k = (u128)1 << (8 * bytes - 1);
        else { x ^= x << 13; x ^= x >> 7; x ^= x << 17; k = ((u128)x << 64) | (x * 0x2545f4914f6cdd1dull); if (bytes == 8) k &= ~0ull; }
        memcpy(rec, &k, (size_t)bytes);
        const int bad = check_digits(rec, bytes, c);
        if (bad) { printf("digits %d %d %d: %d\n", bytes, c, e, bad); return 1; }
      }
    }
    const int64_t ns[] = {1, 64, 4097, 1 << 16, 1 << 20, 3 << 20};
    for (int64_t n : ns) {
      const int c = n >= (3 << 20) ? 16 : (n >= (1 << 19) ? 14 : 12);
      const int64_t in[11] = {n, c, 256, 4, -1, -1, -1, -1, -1, -1, B};
      int64_t out[64]; uint64_t off[64], sz[64]; int fold[48], consts[16];
      const int nr = sim_msm_plan(in, out, off, sz, fold, consts);
      uint64_t end = 0;
      for (int r = 0; r < nr; ++r) {
        if (off[r] < end || off[r] + sz[r] > (uint64_t)out[39]) { printf("plan %d %lld region %d\n", bytes, (long long)n, r); return 1; }
        end = off[r] + sz[r];
      }
    }
  }
  printf("MSM_SHORT_SIM_OK\n");
  return 0;
}
#endif
