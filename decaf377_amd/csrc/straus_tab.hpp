// straus_tab.hpp -- the device side the Straus-chain kernels share (batch_msm.hip, batch_msm_long.hip, batch_msm_mixed.hip;
// batch_msm_long_indexed.hip takes StrausTab and keeps its own gathered copy of the wave chain): the per-lane table scratch of
// the lane kernels and the wave-per-sum chain.  Not part of straus.hpp, which the host simulation compiles: the table is stored
// with slot_store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "curve.hpp"
#include "device_util.hpp"
#include "quad_ops.hpp"
#include "row_ops.hpp"
#include "straus.hpp"

namespace d377 {

// Scratch of one resident lane: tables [point][entry][lane] of four 12-word limb slots (BM_ENTRY_WORDS, 192 bytes: the
// layout k_scalar_mul_var had before its entries became 128-byte packed records; a wave stores one entry as 12 KiB
// contiguous; a negative digit swaps the ypx / ymx slots by address), and the digit words [window][lane]: nibble p of word w =
// the signed digit of point p in window w.  The area is per device (batch_host.hpp: straus_scratch_reserve).
struct StrausTab {
  uint32_t* tab;
  uint32_t* dig;
  size_t nthreads, tid;
  __device__ __forceinline__ uint32_t* entry(int p, int j) const { return tab + (((size_t)p * VB_ENTRIES + j) * nthreads + tid) * BM_ENTRY_WORDS; }
  __device__ __forceinline__ void store(int p, int j, const gec& c) {
    uint32_t* q = entry(p, j);
    slot_store(q, c.ypx); slot_store(q + SLOT, c.ymx); slot_store(q + 2 * SLOT, c.z2); slot_store(q + 3 * SLOT, c.kt);
  }
  __device__ __forceinline__ gec load(int p, int j, bool swap) const {
    const uint32_t* q = entry(p, j);
    gec c;
    c.ypx = slot_load(q + (swap ? SLOT : 0));
    c.ymx = slot_load(q + (swap ? 0 : SLOT));
    c.z2 = slot_load(q + 2 * SLOT);
    c.kt = slot_load(q + 3 * SLOT);
    return c;
  }
  __device__ __forceinline__ void dig_store(int w, uint32_t v) { dig[(size_t)w * nthreads + tid] = v; }
  __device__ __forceinline__ uint32_t dig_load(int w) const { return dig[(size_t)w * nthreads + tid]; }
};

// ---- one wave per sum: the chain in the lane-spread form (row_ops.hpp), as msm.hip's k_msm_tiny, m tables in LDS --------------
// the square roots of a group of Encodings keep their POW_TAB odd powers (64 words each) in the table of the group's first
// point, which is built after them
static_assert(POW_TAB * 64 <= row::RQ_TAB_ENTRIES * row::RQ_WORDS, "row_sqrt_powers' scratch must fit in one point's LDS table");

// The workgroup (one wave) sums the m <= 8 terms from `first` on -> [1/2] of the sum, in every lane (the caller stores the
// double).  LDS of the caller: tab = m tables of RQ_TAB_ENTRIES x RQ_WORDS words, xrec = 2 x RQ_WORDS words, sdg = the points'
// signed digits (wave-uniform reads in the loop).  status: one byte per term of the Encoding form.
template <bool ENCODED>
__device__ __forceinline__ ge straus_wave_sum(const SqrtTables& T, const void* pts_in, const uint8_t* scalar32, size_t first, int m,
                                              uint8_t* status, uint32_t* tab, uint32_t* xrec, uint32_t (*sdg)[8]) {
  using row::RQ_WORDS;
  const int t = threadIdx.x;
  const row::RowK K = row::row_consts();
  const row::RowSel S = row::row_sel();
  // points in groups of four: lane t looks after point base + (t & 3) of the group (the square roots of Encodings run their
  // power chains on the four rows of the wave, one point per row)
#pragma unroll 1
  for (int base = 0; base < m; base += 4) {
    const int pj = t & 3;
    const bool mine = base + pj < m;
    const size_t e_mine = first + (size_t)(mine ? base + pj : 0);
    ge g;
    bool skip = !mine;
    if (ENCODED) {
      uint32_t w[8];
      load32(reinterpret_cast<const uint8_t*>(pts_in), e_mine, w);
      if (t < 4) row::row_store_from_fe(xrec + 16 * t, ge_decompress_den(w));
      __syncthreads();
      const row::RowPowers pw = row::row_sqrt_powers(xrec[t], tab + base * row::RQ_TAB_ENTRIES * RQ_WORDS, t, K);   // (this group's tables: not built yet)
      __syncthreads();
      xrec[t] = pw.v; xrec[RQ_WORDS + t] = pw.uv;
      __syncthreads();
      const fe pv = row::row_load_to_fe(xrec + 16 * pj), puv = row::row_load_to_fe(xrec + RQ_WORDS + 16 * pj);
      __syncthreads();
      const uint32_t bad = ge_decompress_from_powers(T, w, pv, puv, &g);
      if (t < 4 && mine) status[e_mine] = (uint8_t)bad;
      skip |= bad != 0;
    } else {
      g = load_ge_mont256(reinterpret_cast<const uint64_t*>(pts_in), e_mine);
      skip |= fe_is_zero(g.z);
      D377_INVARIANT(T, g, t < 4 && !skip);
    }
#pragma unroll 1
    for (int j = 0; j < 4 && base + j < m; ++j) {
      uint32_t k[8], dg[8];
      load32(scalar32, first + (size_t)(base + j), k);
      fr_reduce_words(k);
      fr_half_words(k);
      fr_recode_signed16(k, dg);
      if (pj == j && t < 16) row::row_store_from_fe(xrec + 16 * (t >> 2), fe_pick(t >> 2, g.x, g.y, g.z, g.t));
      __syncthreads();
      const bool dead = __shfl((int)skip, j) != 0;                  // (wave-uniform: lane j's verdict on point base + j)
      if (t < 8) sdg[base + j][t] = dead ? 0u : dg[t];              // dead: every digit 0
      row::rq_build_table(dead ? row::rq_identity(S) : xrec[t], tab + (base + j) * row::RQ_TAB_ENTRIES * RQ_WORDS, S, K);
      __syncthreads();
    }
  }
  uint32_t v = row::rq_identity(S);
#pragma unroll 1
  for (int i = 63; i >= 0; --i) {
    if (i != 63) {
#pragma unroll 1
      for (int k = 0; k < 4; ++k) v = row::rq_double_neg(v, S, K);  // four sign-folded doublings keep the sign
    }
#pragma unroll 1
    for (int j = 0; j < m; ++j) {
      const int d = fr_digit(sdg[j], i);
      if (d != 0) v = row::rq_add(v, tab + (j * row::RQ_TAB_ENTRIES + (d < 0 ? -d : d)) * RQ_WORDS, S, d < 0, K);
    }
  }
  __syncthreads();
  xrec[t] = v;
  __syncthreads();
  return row::rq_load_point(xrec);
}

}  // namespace d377
