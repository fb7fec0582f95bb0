// Test-only host build of d377_batch_fixed_long_msm (decaf377_amd/csrc/fixed_bases.hip): the cut of fixed_msm_long_plan.hpp,
// over it k_fixed_msm_seg's walk -- every segment the device's own multi-comb walk (curve.hpp: ge_fixed_msm_w8) through a table
// wrapper that offsets the comb index by the segment's first base, with the kernel's scalar loader -- the partial sums written
// as Element records (the double of the walk's result), the fold levels with the records' own addition (ge_add_raw_words, what
// k_msm_long_fold runs) and the chunked compressor's pass on the last level's records.  One segment per sum is the lane
// kernel's walk (as fixed_bases_sim.cpp runs it), as on the device.  NOT part of the product: compiled by
// tests/test_fixed_msm_long_host.py with g++, it exists only under tests/.  It includes sim.cpp (sim_init, the round structure
// of dcb_rounds, the record I/O).
//
// With -DFML_SIM_MAIN it is a stand-alone program (the sanitizer build):
//   fixed_msm_long_sim IN OUT m n L bits     IN: m x 128 bytes of bases, then n x m x 32 bytes of scalars;
//                                            OUT: n x 32 bytes of Encodings, then n x 128 bytes of Element records
#include "sim.cpp"
#include "fixed_msm_long_plan.hpp"

namespace {

// The combs of the m bases, entry by entry ON DEMAND: a sum touches W of a comb's W x (2^(BITS-1) + 1) records, and the combs of
// 257 bases at 12 bits would be 1.2 GB.  Entry c of window i of base j is c * 2^(BITS i) * B_j in affine cached form, the
// record k_fb_window_bases + k_init_fbase store (fixed_comb.hpp); the window bases are made once.
std::vector<ge> g_wb;                                               // [j W + i] = 2^(BITS i) B_j
int g_fx_bits = 0, g_fx_m = 0;

template <int BITS>
struct LazyCombTabs {
  gea load(int j, int i, int c, bool swap) const {
    const ge& base = g_wb[(size_t)j * FbShape<BITS>::windows + i];
    ge acc = ge_identity();
    for (int b = BITS - 1; b >= 0; --b) {
      acc = ge_double(acc);
      if ((c >> b) & 1) acc = ge_add(acc, base);
    }
    const fe zi = fe_invert(acc.z);
    const gea r = gea_from_affine(fe_mul(acc.x, zi), fe_mul(acc.y, zi));
    gea g;
    g.ypx = swap ? r.ymx : r.ypx; g.ymx = swap ? r.ypx : r.ymx; g.kt = r.kt;
    fe_assume_carried(g.ypx, 26.0); fe_assume_carried(g.ymx, 26.0); fe_assume_carried(g.kt, 9.0);
    return g;
  }
};

template <int BITS>
void build(const uint32_t* xyzt, int m) {
  constexpr int W = FbShape<BITS>::windows;
  g_wb.assign((size_t)m * W, ge_identity());
  for (int j = 0; j < m; ++j) {
    ge p = ge_load256(xyzt + 32 * j);
    if (fe_is_zero(p.z)) p = ge_identity();                        // a record with Z = 0 counts as the identity
    for (int i = 0; i < W; ++i) {
      g_wb[(size_t)j * W + i] = p;
      for (int b = 0; b < BITS; ++b) p = ge_double(p);
    }
  }
}

template <class FTab>
struct HostOffsetTabs {
  const FTab& tabs;
  int first;
  gea load(int j, int i, int c, bool swap) const { return tabs.load(first + j, i, c, swap); }
};

// one segment per sum: k_fixed_msm_lane's walk, the half point into the square-root-free compressor (as fixed_bases_sim.cpp)
template <int BITS>
void run_lane(const uint32_t* k, size_t n, uint32_t* enc, uint32_t* xyzt_out) {
  const LazyCombTabs<BITS> ft{};
  const int m = g_fx_m;
  dcb_rounds<0>(n, enc, true,
    [&](HostDcbIO&, size_t, int) {},
    [&](HostDcbIO& io, size_t i, int j) {
      const ge r = ge_fixed_msm_w8<BITS>(m, [&](int p, uint32_t kk[8]) {
        memcpy(kk, k + 8 * (i * (size_t)m + (size_t)p), 32);
        fr_reduce_words(kk);
        fr_half_words(kk);
      }, ft, DCB_WANT_T);
      if (xyzt_out) ge_store256(ge_double_fast(r, true), xyzt_out + 32 * i);
      dcb_put(io, j, ge_dcb_from_half(r, false));
    });
}

template <int BITS>
void run_long(const uint32_t* k, size_t n, const FixedLongPlan& plan, uint32_t* enc, uint32_t* xyzt_out) {
  const LazyCombTabs<BITS> ft{};
  const size_t total = n * plan.g;
  std::vector<uint32_t> cur(total * 32), next;
  for (size_t P = 0; P < total; ++P) {                             // k_fixed_msm_seg's lane P
    const size_t q = P / n, s = P % n;
    const size_t first = s * plan.m + plan.first(q);
    const HostOffsetTabs<LazyCombTabs<BITS>> st{ft, (int)plan.first(q)};
    const ge r = ge_fixed_msm_w8<BITS>((int)plan.count(q), [&](int p, uint32_t kk[8]) {
      memcpy(kk, k + 8 * (first + (size_t)p), 32);
      fr_reduce_words(kk);
      fr_half_words(kk);
    }, st, false);
    ge_store256(ge_double_fast(r, true), cur.data() + 32 * (s * plan.g + q));
  }
  for (size_t c = plan.g; c > 1; c = fold_out(c)) {                // k_msm_long_fold, level by level
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
  sim_compress_assisted(cur.data(), n, enc);                       // k_compress_chunked's rounds
}

}  // namespace

extern "C" {

// the cut for the Python side: out = {g, b, first(q) and count(q) for q < g ...} (2 + 2 g words)
void fml_plan(size_t m, size_t n, size_t L, size_t* out) {
  const FixedLongPlan p = fixed_long_plan(m, n, L);
  out[0] = p.g; out[1] = p.b;
  for (size_t q = 0; q < p.g; ++q) { out[2 + 2 * q] = p.first(q); out[3 + 2 * q] = p.count(q); }
}
size_t fml_seg_min() { return FML_SEG_MIN; }
// how many fold levels g records per sum take
int fml_levels(size_t g) {
  int n = 0;
  for (size_t c = g; c > 1; c = fold_out(c)) ++n;
  return n;
}

// bases: m Element records (32 words each); bits: 8 or 12
int fml_build(const uint32_t* xyzt, int m, int bits) {
  g_fx_m = m;
  g_fx_bits = bits;
  if (bits == 8) build<8>(xyzt, m);
  else if (bits == 12) build<12>(xyzt, m);
  else return -1;
  return 0;
}
// n sums over the bases of fml_build on a device of L resident lanes: k n x m scalars; enc n x 8 words, xyzt_out n x 32 words or
// null; gb (or null): the cut's g and b
int fml_msm_long(const uint32_t* k, size_t n, size_t L, uint32_t* enc, uint32_t* xyzt_out, size_t* gb) {
  if (n == 0 || g_fx_m < 1) return -1;
  const FixedLongPlan plan = fixed_long_plan((size_t)g_fx_m, n, L);
  if (gb) { gb[0] = plan.g; gb[1] = plan.b; }
  if (g_fx_bits == 8) { if (plan.g == 1) run_lane<8>(k, n, enc, xyzt_out); else run_long<8>(k, n, plan, enc, xyzt_out); }
  else if (g_fx_bits == 12) { if (plan.g == 1) run_lane<12>(k, n, enc, xyzt_out); else run_long<12>(k, n, plan, enc, xyzt_out); }
  else return -1;
  return 0;
}

}

#ifdef FML_SIM_MAIN
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
  if (argc != 7) { fprintf(stderr, "usage: %s IN OUT m n L bits\n", argv[0]); return 2; }
  const size_t m = strtoul(argv[3], nullptr, 10), n = strtoul(argv[4], nullptr, 10), L = strtoul(argv[5], nullptr, 10);
  const int bits = atoi(argv[6]);
  if (m < 1 || m > 4096 || n < 1) return 2;
  std::vector<uint32_t> bases(m * 32), k(n * m * 8), out(n * 8 + n * 32);
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  const bool ok = fread(bases.data(), 128, m, f) == m && fread(k.data(), 32, n * m, f) == n * m;
  fclose(f);
  if (!ok) return 3;
  if (sim_init() != 0) return 4;
  if (fml_build(bases.data(), (int)m, bits) != 0) return 4;
  size_t gb[2];
  if (fml_msm_long(k.data(), n, L, out.data(), out.data() + n * 8, gb) != 0) return 5;
  f = fopen(argv[2], "wb");
  if (!f) return 3;
  fwrite(out.data(), 4, out.size(), f);
  fclose(f);
  printf("%zu %zu\n", gb[0], gb[1]);
  return 0;
}
#endif
