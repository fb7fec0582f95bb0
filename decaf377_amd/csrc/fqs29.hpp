// fqs29.hpp -- Fq with signed limbs: the field type of the variable-base window loop.
//
// Same 9 x 29-bit limbs, Montgomery R = 2^261 and constants as fq29.hpp's `fe`; the limbs are int32 and the
// value may be negative.  What that buys (tools/gen_fe_asm.py, "signed streams"):
//   * the product's column accumulator is a signed 64-bit register: the Montgomery digit is m_k = acc mod 2^29,
//     the reduction subtracts m q (terms m_i * (-q_j), -q_j in SGPRs) and, because q = 1 (mod 2^47), acc - m_k is
//     exactly 2^29 floor(acc / 2^29): one arithmetic shift ends the column, with no m_k * q_0 fold.  Every column
//     costs two non-MAC instructions: 187 / 159 / 160 VALU instructions for mul / sqr / sqr2x (fe: 196 / 168 / 169).
//   * a - b needs no k q offset and no carry pass: one instruction per limb.
// Representation contract (machine-checked: each element carries its signed per-limb interval and its value
// interval in the -DD377_BOUNDS build, and every product checks every column of its stream against +-2^63):
//   product:  output of fe_mul / fe_sqr / fe_sqr2x on fes: limbs 0..7 in [0, 2^29), a signed top limb,
//             value in (a*b/R - q, a*b/R].
//   operands: every limb an int32; a squaring's operand limbs below 2^30 in magnitude (it doubles them).
// Going from fe to fes is free (fe limbs are below 2^31).  Back to fe: fe_unsigned adds 2q and runs one carry pass
// (the value must be above -2q + 2^233, which a product's is).
#pragma once
#include <type_traits>
#include "fq29.hpp"

namespace d377 {

struct fes {
  int32_t l[NL];
#if defined(D377_BOUNDS)
  int64_t lo[NL], hi[NL];   // worst-case limb intervals over all inputs
  double vlo, vhi;          // worst-case value interval in units of q
#endif
};

// 2q in radix 2^29, limbs 0..7 below 2^29 (tests/test_signed_field.py checks the value)
constexpr uint32_t Q2L[NL] = {0x00000002u, 0x01180000u, 0x00000085u, 0x09dbfb40u, 0x16002b35u,
                              0x0d1e5c37u, 0x0ab305a2u, 0x17a68b29u, 0x002556cau};

#if defined(D377_BOUNDS)
// ---- static-bound bookkeeping (host simulation only) ------------------------------------------
inline void sbound_limbs_int32(const fes& a, int64_t lim, const char* what) {
  for (int i = 0; i < NL; ++i) bound_require(a.lo[i] >= -lim && a.hi[i] < lim, what);
}
// every partial sum of every column of the signed stream stays inside [-2^63, 2^63): the carry in, then the limb
// products (SCALE 2: the doubled-limb terms of sqr2x), then the reduction terms m_i * (-q_j), m_i in [0, 2^29)
inline void sbound_product(const fes& a, const fes& b, bool square, int scale) {
  sbound_limbs_int32(a, (int64_t)1 << 31, "signed product: operand limb outside int32");
  sbound_limbs_int32(b, (int64_t)1 << 31, "signed product: operand limb outside int32");
  if (square) sbound_limbs_int32(a, (int64_t)1 << 30, "signed square: doubled limb outside int32");
  const __int128 lim = (__int128)1 << 63;
  __int128 clo = 0, chi = 0;                          // carry-in interval
  for (int k = 0; k < 2 * NL - 1; ++k) {
    __int128 lo = clo, hi = chi;                      // reachable partial sums: each term's negative / positive side
    __int128 slo = clo, shi = chi;                    // the column's final sum
    for (int i = 0; i < NL; ++i) {
      const int j = k - i;
      if (j < 0 || j >= NL) continue;
      const __int128 c[4] = {(__int128)a.lo[i] * b.lo[j], (__int128)a.lo[i] * b.hi[j],
                             (__int128)a.hi[i] * b.lo[j], (__int128)a.hi[i] * b.hi[j]};
      __int128 pmin = c[0], pmax = c[0];
      for (int t = 1; t < 4; ++t) { if (c[t] < pmin) pmin = c[t]; if (c[t] > pmax) pmax = c[t]; }
      pmin *= scale; pmax *= scale;
      slo += pmin; shi += pmax;
      if (pmin < 0) lo += pmin;
      if (pmax > 0) hi += pmax;
      if (j >= 1 && i < NL) {
        const __int128 red = -(__int128)MASK29 * QL[j];
        slo += red; lo += red;
      }
    }
    bound_require(lo >= -lim && hi < lim, "signed product column leaves +-2^63");
    // acc >> 29 (arithmetic): floor division
    clo = slo >= 0 ? slo >> RB : -((-slo + MASK29) >> RB);
    chi = shi >= 0 ? shi >> RB : -((-shi + MASK29) >> RB);
  }
}
inline void sbound_set_product(fes& r, const fes& a, const fes& b, double scale) {
  for (int i = 0; i < NL - 1; ++i) { r.lo[i] = 0; r.hi[i] = MASK29; }
  const double p[4] = {a.vlo * b.vlo, a.vlo * b.vhi, a.vhi * b.vlo, a.vhi * b.vhi};
  double pmin = p[0], pmax = p[0];
  for (int t = 1; t < 4; ++t) { if (p[t] < pmin) pmin = p[t]; if (p[t] > pmax) pmax = p[t]; }
  r.vlo = scale * pmin / R_OVER_Q - 1.0 - 1e-6;       // (T - m q) / R with 0 <= m < R
  r.vhi = scale * pmax / R_OVER_Q + 1e-6;
  r.lo[NL - 1] = (int64_t)__builtin_floor(r.vlo * Q_TOP) - 1;     // top = floor(value / 2^232)
  r.hi[NL - 1] = (int64_t)__builtin_floor(r.vhi * Q_TOP) + 1;
  bound_require(r.lo[NL - 1] >= -((int64_t)1 << 31) && r.hi[NL - 1] < ((int64_t)1 << 31), "signed product: top limb outside int32");
}
inline void sbound_linear(fes& r, const char* what) { sbound_limbs_int32(r, (int64_t)1 << 31, what); }
#endif

// ---- multiplication -----------------------------------------------------------------------------
// What the signed streams compute, statement for statement (the host simulation runs these).  The accumulator is
// kept as uint64_t (two's complement, no signed-overflow UB) and shifted arithmetically.
template <bool SCALE2, bool SQUARE>
D377_HD fes fes_mul_ref(const fes& a, const fes& b) {
  uint64_t acc = 0;
  int32_t m[NL], a2[NL], b2[NL];
  fes r;
#pragma unroll
  for (int i = 0; i < NL; ++i) { a2[i] = (int32_t)((uint32_t)a.l[i] << 1); b2[i] = SCALE2 ? a2[i] : a.l[i]; }
#pragma unroll
  for (int k = 0; k < 2 * NL - 1; ++k) {
    const int lo = k < NL ? 0 : k - (NL - 1), hi = k < NL ? k : NL - 1;
    if (SQUARE) {
#pragma unroll
      for (int i = lo; 2 * i < k; ++i) acc += (uint64_t)((int64_t)a2[i] * b2[k - i]);
      if ((k & 1) == 0) acc += (uint64_t)((int64_t)b2[k / 2] * a.l[k / 2]);
    } else {
#pragma unroll
      for (int i = lo; i <= hi; ++i) acc += (uint64_t)((int64_t)a.l[i] * b.l[k - i]);
    }
#pragma unroll
    for (int i = lo; i < (k < NL ? k : NL); ++i) acc -= (uint64_t)((int64_t)m[i] * (int64_t)QL[k - i]);
    if (k < NL) m[k] = (int32_t)((uint32_t)acc & MASK29);
    else r.l[k - NL] = (int32_t)((uint32_t)acc & MASK29);
    acc = (uint64_t)((int64_t)acc >> RB);
  }
  r.l[NL - 1] = (int32_t)(uint32_t)acc;
  return r;
}

#if defined(__HIP_DEVICE_COMPILE__)
// the signed streams take fq29.hpp's operand lists (same numbering) with -q_1 .. -q_8 in SGPRs
#define D377_ASM_NQ                                                                                     \
  "s"(-(int32_t)QL[1]), "s"(-(int32_t)QL[2]), "s"(-(int32_t)QL[3]), "s"(-(int32_t)QL[4]), "s"(-(int32_t)QL[5]), \
  "s"(-(int32_t)QL[6]), "s"(-(int32_t)QL[7]), "s"(-(int32_t)QL[8])
#endif

D377_HD fes fe_mul(const fes& a, const fes& b) {
  D377_B(sbound_product(a, b, false, 1); ++op_counts().mul);
#if defined(__HIP_DEVICE_COMPILE__)
  fes r; int64_t top; int32_t m8;
  asm(D377_ASM_SMUL : D377_ASM_OUT(r, top, m8) : D377_ASM_IN(a), D377_ASM_IN(b), D377_ASM_NQ : D377_ASM_CLOBBER);
  r.l[NL - 1] = (int32_t)top;
#else
  fes r = fes_mul_ref<false, false>(a, b);
#endif
  D377_B(sbound_set_product(r, a, b, 1.0));
  return r;
}
D377_HD fes fe_sqr(const fes& a) {
  D377_B(sbound_product(a, a, true, 1); ++op_counts().sqr);
#if defined(__HIP_DEVICE_COMPILE__)
  fes r; int64_t top; int32_t m8, t[8];
  asm(D377_ASM_SSQR : D377_ASM_OUT(r, top, m8), D377_ASM_TMP8(t) : D377_ASM_IN(a), D377_ASM_NQ : D377_ASM_CLOBBER);
  r.l[NL - 1] = (int32_t)top;
#else
  fes r = fes_mul_ref<false, true>(a, a);
#endif
  D377_B(sbound_set_product(r, a, a, 1.0));
  return r;
}
D377_HD fes fe_sqr2x(const fes& a) {     // 2 a^2
  D377_B(sbound_product(a, a, true, 2); ++op_counts().sqr);
#if defined(__HIP_DEVICE_COMPILE__)
  fes r; int64_t top; int32_t m8, t[8], t8;
  asm(D377_ASM_SSQR2X : D377_ASM_OUT(r, top, m8), D377_ASM_TMP8(t), "=&v"(t8) : D377_ASM_IN(a), D377_ASM_NQ : D377_ASM_CLOBBER);
  r.l[NL - 1] = (int32_t)top;
#else
  fes r = fes_mul_ref<true, true>(a, a);
#endif
  D377_B(sbound_set_product(r, a, a, 2.0));
  return r;
}

// ---- linear operations (limb-wise; none carries) ----------------------------------------------
// (the limb arithmetic wraps as uint32: in range it is the int32 arithmetic the bounds build proves)
D377_HD fes fe_add(const fes& a, const fes& b) {
  fes r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = (int32_t)((uint32_t)a.l[i] + (uint32_t)b.l[i]);
#if defined(D377_BOUNDS)
  for (int i = 0; i < NL; ++i) { r.lo[i] = a.lo[i] + b.lo[i]; r.hi[i] = a.hi[i] + b.hi[i]; }
  r.vlo = a.vlo + b.vlo; r.vhi = a.vhi + b.vhi;
  sbound_linear(r, "signed fe_add limb leaves int32");
#endif
  return r;
}
D377_HD fes fe_sub(const fes& a, const fes& b) {
  fes r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = (int32_t)((uint32_t)a.l[i] - (uint32_t)b.l[i]);
#if defined(D377_BOUNDS)
  for (int i = 0; i < NL; ++i) { r.lo[i] = a.lo[i] - b.hi[i]; r.hi[i] = a.hi[i] - b.lo[i]; }
  r.vlo = a.vlo - b.vhi; r.vhi = a.vhi - b.vlo;
  sbound_linear(r, "signed fe_sub limb leaves int32");
#endif
  return r;
}
D377_HD fes fe_sub_nc(const fes& a, const fes& b) { return fe_sub(a, b); }   // (fe's name for the uncarried difference)
D377_HD fes fe_neg(const fes& a) {
  fes r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = (int32_t)(0u - (uint32_t)a.l[i]);
#if defined(D377_BOUNDS)
  for (int i = 0; i < NL; ++i) { r.lo[i] = -a.hi[i]; r.hi[i] = -a.lo[i]; }
  r.vlo = -a.vhi; r.vhi = -a.vlo;
  sbound_linear(r, "signed fe_neg limb leaves int32");
#endif
  return r;
}
D377_HD fes fe_dbl(const fes& a) { return fe_add(a, a); }

// one parallel carry pass with arithmetic shifts: limbs 0..7 back to [carry_lo, 2^29 + carry_hi), value unchanged
D377_HD fes fe_carry(const fes& a) {
  fes r;
  r.l[0] = (int32_t)((uint32_t)a.l[0] & MASK29);
#pragma unroll
  for (int i = 1; i < NL - 1; ++i) r.l[i] = (int32_t)((uint32_t)a.l[i] & MASK29) + (a.l[i - 1] >> RB);
  r.l[NL - 1] = a.l[NL - 1] + (a.l[NL - 2] >> RB);
#if defined(D377_BOUNDS)
  auto low = [&](int i, int64_t& lo, int64_t& hi) {    // a_i & (2^29 - 1): the interval itself if it is inside [0, 2^29)
    if (a.lo[i] >= 0 && a.hi[i] <= MASK29) { lo = a.lo[i]; hi = a.hi[i]; } else { lo = 0; hi = MASK29; }
  };
  auto sh = [](int64_t v) { return v >= 0 ? v >> RB : -((-v + MASK29) >> RB); };
  low(0, r.lo[0], r.hi[0]);
  for (int i = 1; i < NL; ++i) {
    int64_t lo, hi;
    if (i < NL - 1) low(i, lo, hi); else { lo = a.lo[i]; hi = a.hi[i]; }
    r.lo[i] = lo + sh(a.lo[i - 1]); r.hi[i] = hi + sh(a.hi[i - 1]);
  }
  r.vlo = a.vlo; r.vhi = a.vhi;
  sbound_linear(r, "signed fe_carry top limb leaves int32");
#endif
  return r;
}

D377_HD fes fe_select(bool c, const fes& a, const fes& b) {   // c ? a : b
  fes r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = c ? a.l[i] : b.l[i];
#if defined(D377_BOUNDS)
  for (int i = 0; i < NL; ++i) { r.lo[i] = a.lo[i] < b.lo[i] ? a.lo[i] : b.lo[i]; r.hi[i] = a.hi[i] > b.hi[i] ? a.hi[i] : b.hi[i]; }
  r.vlo = a.vlo < b.vlo ? a.vlo : b.vlo; r.vhi = a.vhi > b.vhi ? a.vhi : b.vhi;
#endif
  return r;
}

// ---- conversions --------------------------------------------------------------------------------
// fe_as<F>(x): an fe as the field type F of a templated formula (fe: itself; fes: the same limbs, free)
D377_HD fes fes_from_fe(const fe& a) {
  fes r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = (int32_t)a.l[i];
#if defined(D377_BOUNDS)
  for (int i = 0; i < NL; ++i) {
    bound_require(a.ub[i] < (1ull << 31), "fe -> fes: limb may not fit int32");
    r.lo[i] = 0; r.hi[i] = (int64_t)a.ub[i];
  }
  r.vlo = 0; r.vhi = a.vq;
#endif
  return r;
}
template <class F>
D377_HD F fe_as(const fe& a) {
  if constexpr (std::is_same<F, fe>::value) return a;
  else return fes_from_fe(a);
}

// back to fe: + 2q, then one carry pass.  Carried result (limbs < 2^29 + 8), value below the input's bound + 2q.
D377_HD fe fe_unsigned(const fe& a) { return a; }
D377_HD fe fe_unsigned(const fes& a) {
  fe t;
#pragma unroll
  for (int i = 0; i < NL; ++i) t.l[i] = (uint32_t)a.l[i] + Q2L[i];
#if defined(D377_BOUNDS)
  for (int i = 0; i < NL; ++i) {
    bound_require(a.lo[i] + (int64_t)Q2L[i] >= 0, "fes -> fe: limb + 2q may be negative");
    t.ub[i] = (uint64_t)(a.hi[i] + (int64_t)Q2L[i]);
    bound_require(t.ub[i] < (1ull << 32), "fes -> fe: limb + 2q overflows 32 bits");
  }
  t.vq = a.vhi + 2.0;
#endif
  return fe_carry(t);
}

// ---- the 256-bit packed form (the variable-base window table's slots: device_util.hpp, d377.hip GlobalTab) ----------
// A table slot holds the element's value as one little-endian integer in [0, 2^256 = 13.7q): 8 words, so that the four
// slots of an entry fill exactly one 128-byte line.  Packing brings the value v into that range by adding 9q or -4q,
// chosen by the top limb alone.  A table entry is a product, a sum or a difference of two products, or -- entry 1, made
// of the point as it was decompressed or loaded -- of two carried fe coordinates (below 8.7q each), so v lies in
// (-8.7q, 17.4q); and with limbs 0..7 below 2^30 in magnitude the top limb is within 2 of v / 2^232.  Top limb below
// PACK_BIG_TOP (v < 4.29q): + 9q, in [0, 13.3q); from there on (v > 4.28q): - 4q, in (0.28q, 13.4q).  The bounds build
// asserts v in [-9q, 17.7q) and the limb magnitudes.  Then the one SEQUENTIAL carry of the chain leaves nine exact
// 29-bit digits, and 9 x 29 bits are cut into 8 x 32.  Unpacking gives limbs 0..7 in [0, 2^29) and a top limb below
// 2^24: tighter than any operand the window loop read before.
constexpr uint32_t Q4L[NL] = {0x00000004u, 0x02300000u, 0x0000010au, 0x13b7f680u, 0x0c00566au,
                              0x1a3cb86fu, 0x15660b44u, 0x0f4d1652u, 0x004aad95u};
constexpr uint32_t Q9L[NL] = {0x00000009u, 0x14ec0000u, 0x00000256u, 0x1c5deaa0u, 0x1300c26fu, 0x1b089efau, 0x0025995au, 0x0a6d723au, 0x00a80690u};
constexpr bool is_multiple_of_q(const uint32_t (&m)[NL], uint64_t k) {
  uint64_t c = 0;
  for (int i = 0; i < NL; ++i) {
    const uint64_t t = k * QL[i] + c;
    if (m[i] != (i < NL - 1 ? (t & MASK29) : t)) return false;
    c = t >> RB;
  }
  return true;
}
static_assert(is_multiple_of_q(Q4L, 4) && is_multiple_of_q(Q9L, 9), "Q4L, Q9L must be 4q and 9q in radix 2^29");
constexpr int PACKED_WORDS = 8;
// the top limb at which the pack turns from + 9q to - 4q: at least 4 q / 2^232 + 3 = 4 894 105 (v - 4q >= 0 above it),
// at most 2^24 - 9 q / 2^232 - 2 = 5 765 486 (v + 9q < 2^256 below it)
constexpr int32_t PACK_BIG_TOP = 5 << 20;

D377_HD void fes_pack256(const fes& a, uint32_t w[PACKED_WORDS]) {
  uint32_t t[NL];
  int32_t c = 0;
  const bool big = a.l[NL - 1] >= PACK_BIG_TOP;
#pragma unroll
  for (int i = 0; i < NL - 1; ++i) {
    const int32_t s = (int32_t)((uint32_t)a.l[i] + (big ? 0u - Q4L[i] : Q9L[i]) + (uint32_t)c);
    t[i] = (uint32_t)s & MASK29;
    c = s >> RB;
  }
  t[NL - 1] = (uint32_t)a.l[NL - 1] + (big ? 0u - Q4L[NL - 1] : Q9L[NL - 1]) + (uint32_t)c;
#if defined(D377_BOUNDS)
  {
    auto sh = [](int64_t v) { return v >= 0 ? v >> RB : -((-v + MASK29) >> RB); };
    int64_t clo = 0, chi = 0;
    for (int i = 0; i < NL; ++i) {
      const int64_t lo = a.lo[i] - (int64_t)Q4L[i] + clo, hi = a.hi[i] + (int64_t)Q9L[i] + chi;
      bound_require(lo >= -((int64_t)1 << 31) && hi < ((int64_t)1 << 31), "fes pack: digit sum leaves int32");
      if (i < NL - 1) bound_require(a.lo[i] > -((int64_t)1 << 30) && a.hi[i] < ((int64_t)1 << 30), "fes pack: a low limb may reach 2^30: the top limb no longer tells the value");
      clo = sh(lo); chi = sh(hi);
    }
    bound_require(a.vlo + 9.0 >= 0.0, "fes pack: value + 9q may be negative");
    bound_require(a.vhi - 4.0 < R_OVER_Q / 32.0, "fes pack: value - 4q may reach 2^256");
    bound_require(t[NL - 1] < (1u << 24), "fes pack: top digit outside [0, 2^24)");   // (this input's own digit)
  }
#endif
#pragma unroll
  for (int j = 0; j < PACKED_WORDS; ++j) w[j] = (t[j] >> (3 * j)) | (t[j + 1] << (RB - 3 * j));
}
D377_HD fes fes_unpack256(const uint32_t w[PACKED_WORDS]) {
  fes r;
  r.l[0] = (int32_t)(w[0] & MASK29);
#pragma unroll
  for (int i = 1; i < NL - 1; ++i) r.l[i] = (int32_t)(((w[i - 1] >> (32 - 3 * i)) | (w[i] << (3 * i))) & MASK29);
  r.l[NL - 1] = (int32_t)(w[PACKED_WORDS - 1] >> 8);
#if defined(D377_BOUNDS)
  for (int i = 0; i < NL - 1; ++i) { r.lo[i] = 0; r.hi[i] = MASK29; }
  r.lo[NL - 1] = 0; r.hi[NL - 1] = (1 << 24) - 1;
  r.vlo = 0.0; r.vhi = R_OVER_Q / 32.0;               // any value below 2^256
#endif
  return r;
}

}  // namespace d377
