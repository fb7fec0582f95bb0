// Test-only host build of the signed-limb field type (decaf377_amd/csrc/fqs29.hpp) and of the variable-base chain
// instantiated on it (curve.hpp, ge_scalar_mul_w4<fes>), next to the unsigned chain of sim.cpp.  Compiled by
// tests/test_signed_field.py with g++ (once plain, once with -DD377_BOUNDS); nothing in decaf377_amd/ loads it.
#include "sim.cpp"

namespace {
// the per-lane table of the signed chain (d377.hip GlobalTab<fes>): a negative digit swaps ypx / ymx.  In the bounds
// build both slots carry the union of the two bounds, so a walk proves either order.
struct HostTabS {
  gec_of<fes> e[9];
  void store(int j, const gec_of<fes>& g) {
    e[j] = g;
#if defined(D377_BOUNDS)
    const fes u = fe_select(false, g.ypx, g.ymx);      // (select's bounds are the union of both)
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
fes fes_in(const int32_t* w) {       // test operands: their own limbs as the bounds
  fes a;
  for (int i = 0; i < NL; ++i) a.l[i] = w[i];
#if defined(D377_BOUNDS)
  for (int i = 0; i < NL; ++i) { a.lo[i] = w[i]; a.hi[i] = w[i]; }
  a.vlo = -1e9; a.vhi = 1e9;
#endif
  return a;
}
}  // namespace

extern "C" {
void sims_consts(uint32_t* q2l) { for (int i = 0; i < NL; ++i) q2l[i] = Q2L[i]; }

// op 0: a*b/R, 1: a^2/R, 2: 2a^2/R, 3: fe_carry(a), 4: a - b, 5: fe_unsigned(a) (as uint32 limbs); n rows of 9 limbs
void sims_field_op(int op, const int32_t* a, const int32_t* b, size_t n, int32_t* r) {
  for (size_t i = 0; i < n; ++i) {
    const fes x = fes_in(a + 9 * i), y = fes_in(b + 9 * i);
    fes z;
    if (op == 0) z = fes_mul_ref<false, false>(x, y);
    else if (op == 1) z = fes_mul_ref<false, true>(x, x);
    else if (op == 2) z = fes_mul_ref<true, true>(x, x);
    else if (op == 3) z = fe_carry(x);
    else if (op == 4) z = fe_sub(x, y);
    else { const fe u = fe_unsigned(x); for (int k = 0; k < NL; ++k) z.l[k] = (int32_t)u.l[k]; }
    for (int k = 0; k < NL; ++k) r[9 * i + k] = z.l[k];
  }
}

// d377_batch_scalar_mul_var's lane (k_scalar_mul_var) with the signed window loop: sim_scalar_mul_var's twin
void sims_scalar_mul_var(const uint32_t* enc, const uint32_t* k, size_t n, uint32_t* out, uint8_t* st) {
  dcb_rounds<1>(n, out, true,
    [&](HostDcbIO& io, size_t i, int j) { dcb_put_den(io, 0, j, ge_decompress_den(enc + 8 * i)); },
    [&](HostDcbIO& io, size_t i, int j) {
      const fe inv = dcb_get_inv(io, 0, j);
      RegPowTab pt; ge g; uint32_t bad = ge_decompress(g_T, pt, enc + 8 * i, &g, &inv);
      st[i] = (uint8_t)bad;
      uint32_t kk[8], dg[8]; memcpy(kk, k + 8 * i, 32); fr_reduce_words(kk); fr_half_words(kk); fr_recode_signed16(kk, dg);
      HostTabS tab; ge r = ge_scalar_mul_w4<fes>(g, dg, tab, DCB_WANT_T);
      dcb_put(io, j, ge_dcb_from_half(r, bad != 0));
    });
}
// the chain with T wanted (k_scalar_mul_var_el's use) and the square-root compressor: sim_scalar_mul_var_sqrt's twin
void sims_scalar_mul_var_sqrt(const uint32_t* enc, const uint32_t* k, size_t n, uint32_t* out, uint8_t* st) {
  for (size_t i = 0; i < n; ++i) {
    RegPowTab pt; ge g; uint32_t bad = ge_decompress(g_T, pt, enc + 8 * i, &g);
    st[i] = (uint8_t)bad;
    if (bad) { memset(out + 8 * i, 0, 32); continue; }
    uint32_t kk[8], dg[8]; memcpy(kk, k + 8 * i, 32); fr_reduce_words(kk); fr_recode_signed16(kk, dg);
    HostTabS tab; ge r = ge_scalar_mul_w4<fes>(g, dg, tab);
    ge_compress(g_T, pt, r, out + 8 * i);
  }
}
}
