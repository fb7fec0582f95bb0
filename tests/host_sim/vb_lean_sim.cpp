// Test-only host build of the chain k_scalar_mul_var / k_scalar_mul_var_el run (curve.hpp: ge_scalar_mul_w4_lean -- 62
// windows from a start value lifted from table entry d62, 2XY from a squaring) next to the reference statement it replaced
// in those kernels (ge_scalar_mul_w4<fes>).  Compiled by tests/test_vb_lean_host.py with g++ (once plain, once with
// -DD377_BOUNDS) and included by the stand-alone program tests/cpp/vb_lean_chain.cpp; nothing in decaf377_amd/ loads it.
// It reuses vb_signed_sqrt_sim.cpp (the signed square root's harness and the limb table with a shared identity), which
// includes sim.cpp.
#include "vb_signed_sqrt_sim.cpp"

namespace {
// the limb table that stores its own entry 0 (signed_sim.cpp's HostTabS): the chain's store(0, identity) branch
struct LeanTabOwnId {
  gec_of<fes> e[9];
  void store(int j, const gec_of<fes>& g) {
    e[j] = g;
#if defined(D377_BOUNDS)
    const fes u = fe_select(false, g.ypx, g.ymx);      // both swappable slots carry the union of the two bounds
    for (int i = 0; i < NL; ++i) { e[j].ypx.lo[i] = e[j].ymx.lo[i] = u.lo[i]; e[j].ypx.hi[i] = e[j].ymx.hi[i] = u.hi[i]; }
    e[j].ypx.vlo = e[j].ymx.vlo = u.vlo; e[j].ypx.vhi = e[j].ymx.vhi = u.vhi;
#endif
  }
  gec_of<fes> load(int j, bool swap) const {
    gec_of<fes> c = e[j];
    if (swap) { const fes t = c.ypx; c.ypx = c.ymx; c.ymx = t; }
    return c;
  }
};
// d377.hip GlobalTab on the host (tests/cpp/vb_packed_table.cpp's HostTabPacked): four packed 256-bit slots per entry,
// entry 0 the shared packed identity that nobody stores
unsigned long g_lean_store0 = 0;
struct LeanTabPacked {
  static constexpr bool shared_identity = true;
  uint32_t e[9][4 * PACKED_WORDS];
  LeanTabPacked() { put(0, gec_identity<fes>()); }
  void put(int j, const gec_of<fes>& g) {
    fes_pack256(g.ypx, e[j]); fes_pack256(g.ymx, e[j] + PACKED_WORDS);
    fes_pack256(g.z2, e[j] + 2 * PACKED_WORDS); fes_pack256(g.kt, e[j] + 3 * PACKED_WORDS);
  }
  void store(int j, const gec_of<fes>& g) {
    if (j == 0) { ++g_lean_store0; return; }
    put(j, g);
  }
  gec_of<fes> load(int j, bool swap) const {
    const uint32_t* p = e[j];
    gec_of<fes> c;
    c.ypx = fes_unpack256(p + (swap ? PACKED_WORDS : 0));
    c.ymx = fes_unpack256(p + (swap ? 0 : PACKED_WORDS));
    c.z2 = fes_unpack256(p + 2 * PACKED_WORDS);
    c.kt = fes_unpack256(p + 3 * PACKED_WORDS);
    return c;
  }
};

// chain 0: ge_scalar_mul_w4<fes> (the reference statement), 1: ge_scalar_mul_w4_lean
template <class Tab>
ge run_chain(int chain, const ge& g, const uint32_t dg[8], bool want_t) {
  Tab tab;
  return chain ? ge_scalar_mul_w4_lean<fes>(g, dg, tab, want_t) : ge_scalar_mul_w4<fes>(g, dg, tab, want_t);
}
// table 0: limbs, own entry 0; 1: limbs, shared identity; 2: packed slots, shared identity
ge run_chain(int chain, int table, const ge& g, const uint32_t dg[8], bool want_t) {
  if (table == 0) return run_chain<LeanTabOwnId>(chain, g, dg, want_t);
  if (table == 1) return run_chain<HostTabSharedId>(chain, g, dg, want_t);
  return run_chain<LeanTabPacked>(chain, g, dg, want_t);
}
}  // namespace

extern "C" {
// k_scalar_mul_var's lane: signed square root, the window loop on k / 2 mod r, the compressor without a square root (it
// does not read T: want_t may be either).  Returns the number of store(0) calls the shared-identity tables saw.
unsigned long vbl_scalar_mul_var(int chain, int table, int want_t, const uint32_t* enc, const uint32_t* k, size_t n, uint32_t* out,
                                 uint8_t* st) {
  g_store0 = 0; g_lean_store0 = 0;
  dcb_rounds<1>(n, out, true,
    [&](HostDcbIO& io, size_t i, int j) { dcb_put_den(io, 0, j, ge_decompress_den(enc + 8 * i)); },
    [&](HostDcbIO& io, size_t i, int j) {
      const fe inv = dcb_get_inv(io, 0, j);
      RegPowTabS pt; ge g; const uint32_t bad = ge_decompress<fes>(g_T, pt, enc + 8 * i, &g, &inv);
      st[i] = (uint8_t)bad;
      uint32_t kk[8], dg[8]; memcpy(kk, k + 8 * i, 32); fr_reduce_words(kk); fr_half_words(kk); fr_recode_signed16(kk, dg);
      const ge r = run_chain(chain, table, g, dg, want_t != 0 || DCB_WANT_T);
      dcb_put(io, j, ge_dcb_from_half(r, bad != 0));
    });
  return g_store0 + g_lean_store0;
}
// the chain on the scalar itself with T wanted, through the square-root compressor (which reads T)
unsigned long vbl_scalar_mul_var_sqrt(int chain, int table, const uint32_t* enc, const uint32_t* k, size_t n, uint32_t* out, uint8_t* st) {
  g_store0 = 0; g_lean_store0 = 0;
  for (size_t i = 0; i < n; ++i) {
    RegPowTab pt; ge g; const uint32_t bad = ge_decompress(g_T, pt, enc + 8 * i, &g);
    st[i] = (uint8_t)bad;
    if (bad) { memset(out + 8 * i, 0, 32); continue; }
    uint32_t kk[8], dg[8]; memcpy(kk, k + 8 * i, 32); fr_reduce_words(kk); fr_recode_signed16(kk, dg);
    const ge r = run_chain(chain, table, g, dg, true);
    ge_compress(g_T, pt, r, out + 8 * i);
  }
  return g_store0 + g_lean_store0;
}
// k_scalar_mul_var_el: Elements as Montgomery-256 records (any Z), the scalar itself; the result's encoding
unsigned long vbl_scalar_mul_var_el(int chain, int table, const uint32_t* xyzt, const uint32_t* k, size_t n, uint32_t* out) {
  g_store0 = 0; g_lean_store0 = 0;
  for (size_t i = 0; i < n; ++i) {
    const ge g = ge_load256(xyzt + 32 * i);
    uint32_t kk[8], dg[8]; memcpy(kk, k + 8 * i, 32); fr_reduce_words(kk); fr_recode_signed16(kk, dg);
    const ge r = run_chain(chain, table, g, dg, true);
    RegPowTab pt; ge_compress(g_T, pt, r, out + 8 * i);
  }
  return g_store0 + g_lean_store0;
}
// the two top digits of the recoding the kernels hand the chain: of k / 2 mod r (halve) or of k mod r
void vbl_top_digits(int halve, const uint32_t* k, size_t n, int8_t* d62, int8_t* d63) {
  for (size_t i = 0; i < n; ++i) {
    uint32_t kk[8], dg[8]; memcpy(kk, k + 8 * i, 32); fr_reduce_words(kk); if (halve) fr_half_words(kk); fr_recode_signed16(kk, dg);
    d62[i] = (int8_t)fr_digit(dg, 62); d63[i] = (int8_t)fr_digit(dg, 63);
  }
}
}
