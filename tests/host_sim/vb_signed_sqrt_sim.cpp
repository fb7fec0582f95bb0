// Test-only host build of k_scalar_mul_var's lane as it runs now: the decompression's square root on signed limbs
// (curve.hpp: fe_sqrt_ratio_zeta<.., fes>, ge_decompress<fes>) and the window loop over a table that keeps no entry 0 of
// its own (d377.hip GlobalTab: one shared identity record).  Compiled by tests/test_vb_signed_sqrt_host.py with g++ (once
// plain, once with -DD377_BOUNDS); nothing in decaf377_amd/ loads it.  It reuses sim.cpp's host harness, which it includes.
#include "sim.cpp"

namespace {
// the per-lane table with the shared identity: entries 1..8 are the lane's, entry 0 is one constant record that nobody
// stores.  A store(0) is counted (the tests require zero) and dropped.  In the bounds build both swappable slots carry
// the union of the two bounds, as signed_sim.cpp's table does.
unsigned long g_store0 = 0;
struct HostTabSharedId {
  static constexpr bool shared_identity = true;
  gec_of<fes> e[9];
  HostTabSharedId() { e[0] = gec_identity<fes>(); }
  void store(int j, const gec_of<fes>& g) {
    if (j == 0) { ++g_store0; return; }
    e[j] = g;
#if defined(D377_BOUNDS)
    const fes u = fe_select(false, g.ypx, g.ymx);
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
// the power table of the signed chain on the host (the device's LDS table holds the limbs' bit patterns)
template <class F> struct HostPow { typedef RegPowTab type; };
template <> struct HostPow<fes> { typedef RegPowTabS type; };

template <class F>
void sqrt_rows(const uint32_t* num, const uint32_t* den, size_t n, int with_inv, uint32_t* canon9, uint32_t* root, uint8_t* ws) {
  auto one = [&](size_t i, const fe* inv) {
    typename HostPow<F>::type pt; fe r;
    const bool w = fe_sqrt_ratio_zeta<false, F>(g_T, pt, fe_from_words_mod_order_strict(num + 8 * i),
                                                fe_from_words_mod_order_strict(den + 8 * i), &r, false, inv);
    const fe c = fe_canon(r);
    memcpy(canon9 + 9 * i, c.l, 36);
    fe_to_bytes_words(r, root + 8 * i); ws[i] = w;
  };
  if (with_inv) {
    dcb_rounds<1>(n, root, false,
      [&](HostDcbIO& io, size_t i, int j) { dcb_put_den(io, 0, j, fe_from_words_mod_order_strict(den + 8 * i)); },
      [&](HostDcbIO& io, size_t i, int j) { const fe inv = dcb_get_inv(io, 0, j); one(i, &inv); });
  } else {
    for (size_t i = 0; i < n; ++i) one(i, nullptr);
  }
}
template <class F>
void decompress_rows(const uint32_t* enc, size_t n, uint32_t* xyzt, uint8_t* st) {
  dcb_rounds<1>(n, xyzt, false,
    [&](HostDcbIO& io, size_t i, int j) { dcb_put_den(io, 0, j, ge_decompress_den(enc + 8 * i)); },
    [&](HostDcbIO& io, size_t i, int j) {
      const fe inv = dcb_get_inv(io, 0, j);
      typename HostPow<F>::type pt; ge g; const uint32_t bad = ge_decompress<F>(g_T, pt, enc + 8 * i, &g, &inv);
      st[i] = (uint8_t)bad;
      if (bad) memset(xyzt + 32 * i, 0, 128); else ge_store256(g, xyzt + 32 * i);
    });
}
}  // namespace

extern "C" {
// sqrt_ratio_zeta(num, den) with the chain on fe (signed_ = 0) or fes (1), from the batched inverse (with_inv) or in the
// inversion-free form: the root's canonical limbs (9 words), its bytes and the flag
void vss_sqrt(int signed_, int with_inv, const uint32_t* num, const uint32_t* den, size_t n, uint32_t* canon9, uint32_t* root, uint8_t* ws) {
  if (signed_) sqrt_rows<fes>(num, den, n, with_inv, canon9, root, ws);
  else sqrt_rows<fe>(num, den, n, with_inv, canon9, root, ws);
}
// decompression as k_scalar_mul_var runs it (signed_ = 1) and as every other kernel does (0): Montgomery-256 records
void vss_decompress(int signed_, const uint32_t* enc, size_t n, uint32_t* xyzt, uint8_t* st) {
  if (signed_) decompress_rows<fes>(enc, n, xyzt, st);
  else decompress_rows<fe>(enc, n, xyzt, st);
}
// k_scalar_mul_var's lane: signed square root, signed window loop, shared identity; returns the number of store(0) calls
unsigned long vss_scalar_mul_var(const uint32_t* enc, const uint32_t* k, size_t n, uint32_t* out, uint8_t* st) {
  g_store0 = 0;
  dcb_rounds<1>(n, out, true,
    [&](HostDcbIO& io, size_t i, int j) { dcb_put_den(io, 0, j, ge_decompress_den(enc + 8 * i)); },
    [&](HostDcbIO& io, size_t i, int j) {
      const fe inv = dcb_get_inv(io, 0, j);
      RegPowTabS pt; ge g; const uint32_t bad = ge_decompress<fes>(g_T, pt, enc + 8 * i, &g, &inv);
      st[i] = (uint8_t)bad;
      uint32_t kk[8], dg[8]; memcpy(kk, k + 8 * i, 32); fr_reduce_words(kk); fr_half_words(kk); fr_recode_signed16(kk, dg);
      HostTabSharedId tab; const ge r = ge_scalar_mul_w4<fes>(g, dg, tab, DCB_WANT_T);
      dcb_put(io, j, ge_dcb_from_half(r, bad != 0));
    });
  return g_store0;
}
// k_scalar_mul_var_el's chain (the scalar itself, T wanted) over the same table, through the square-root compressor
unsigned long vss_scalar_mul_var_el(const uint32_t* enc, const uint32_t* k, size_t n, uint32_t* out, uint8_t* st) {
  g_store0 = 0;
  for (size_t i = 0; i < n; ++i) {
    RegPowTab pt; ge g; const uint32_t bad = ge_decompress(g_T, pt, enc + 8 * i, &g);
    st[i] = (uint8_t)bad;
    if (bad) { memset(out + 8 * i, 0, 32); continue; }
    uint32_t kk[8], dg[8]; memcpy(kk, k + 8 * i, 32); fr_reduce_words(kk); fr_recode_signed16(kk, dg);
    HostTabSharedId tab; const ge r = ge_scalar_mul_w4<fes>(g, dg, tab);
    ge_compress(g_T, pt, r, out + 8 * i);
  }
  return g_store0;
}
}
