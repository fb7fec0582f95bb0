// fixed_comb.hpp -- the fixed-base comb builder, shared by the context's generator comb (d377.hip, ensure_comb) and the
// caller-chosen bases of d377_fixed_bases_create (fixed_bases.hip).
//
// A comb is W = FbShape<BITS>::windows windows of FbShape<BITS>::entries affine cached records, window i of base B holding
// j * 2^(BITS i) * B.  m combs lie back to back in one allocation, so the combs of m bases are the layout of ONE comb of
// m x W windows: window w = j W + i is window i of base j, and one launch of k_init_fbase builds them all.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "curve.hpp"
#include "device_util.hpp"

namespace d377 {

// FB[w][j] = j * (window base w) in affine cached form, w < nwin, j < FB_ENTRIES.  A thread builds a RUN of FB_RUN
// consecutive multiples of one window: j0 * base by double-and-add, then one addition of the base per entry; the projective
// coordinates are parked in the entries' own records (27 limbs = a record's 27 words) and the run's Z's are inverted together
// (Montgomery's trick: one divsteps inversion per FB_RUN entries).  ~9 000 instructions per entry; one thread per entry with
// its own ladder from B and its own inversion was ~420 000 at 21-bit windows (12.6 M entries).
// bases: nwin window bases as X, Y, Z, T in 4 x SLOT words each.
constexpr int FB_RUN = 16;
template <int FB_BITS>
__global__ void __launch_bounds__(BLOCK) k_init_fbase(const uint32_t* bases, uint32_t* fb, size_t nwin) {
  constexpr int FB_ENTRIES = FbShape<FB_BITS>::entries;
  constexpr int RUNS = (FB_ENTRIES + FB_RUN - 1) / FB_RUN;
  const size_t idx = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (idx >= nwin * RUNS) return;
  const size_t i = idx / RUNS;
  const int j0 = (int)(idx % RUNS) * FB_RUN;
  ge base;
  base.x = slot_load(bases + i * 4 * SLOT); base.y = slot_load(bases + i * 4 * SLOT + SLOT);
  base.z = slot_load(bases + i * 4 * SLOT + 2 * SLOT); base.t = slot_load(bases + i * 4 * SLOT + 3 * SLOT);
  ge acc = ge_identity();
#pragma unroll 1
  for (int b = FB_BITS - 1; b >= 0; --b) {                     // acc = j0 * base
    acc = ge_double(acc);
    if ((j0 >> b) & 1) acc = ge_add(acc, base);
  }
  uint32_t* rec0 = fb + (i * FB_ENTRIES + j0) * FBW_ENTRY_WORDS;
  fe prefix[FB_RUN];
  fe c = fe_const(FE_ONE);
#pragma unroll
  for (int r = 0; r < FB_RUN; ++r) {
    if (j0 + r < FB_ENTRIES) {
      uint32_t* q = rec0 + (size_t)r * FBW_ENTRY_WORDS;
#pragma unroll
      for (int k = 0; k < NL; ++k) { q[k] = acc.x.l[k]; q[NL + k] = acc.y.l[k]; q[2 * NL + k] = acc.z.l[k]; }
      prefix[r] = c;
      c = fe_mul(c, acc.z);
      acc = ge_add(acc, base);
    }
  }
  fe inv = fe_invert(c);
#pragma unroll
  for (int r = FB_RUN - 1; r >= 0; --r) {
    if (j0 + r < FB_ENTRIES) {
      uint32_t* q = rec0 + (size_t)r * FBW_ENTRY_WORDS;
      fe X, Y, Z;
#pragma unroll
      for (int k = 0; k < NL; ++k) { X.l[k] = q[k]; Y.l[k] = q[NL + k]; Z.l[k] = q[2 * NL + k]; }
      const fe zi = fe_mul(inv, prefix[r]);
      inv = fe_mul(inv, Z);
      pt_store_affine(q, gea_from_affine(fe_mul(X, zi), fe_mul(Y, zi)));
    }
  }
}

// The window bases of m caller-chosen bases: bases[j W + i] = 2^(BITS i) * B_j, one thread per base.  B_j is read from an
// Element record (X, Y, Z, T Montgomery limbs, T Z = X Y); a record with Z = 0 is no group element and counts as the
// identity, whose comb is all identities.
template <int BITS>
__global__ void k_fb_window_bases(const uint64_t* xyzt, int m, uint32_t* bases) {
  constexpr int W = FbShape<BITS>::windows;
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= m) return;
  ge p = load_ge_mont256(xyzt, (size_t)j);
  if (fe_is_zero(p.z)) p = ge_identity();
  uint32_t* out = bases + (size_t)j * W * 4 * SLOT;
#pragma unroll 1
  for (int i = 0; i < W; ++i) {
    slot_store(out + (size_t)i * 4 * SLOT, p.x); slot_store(out + (size_t)i * 4 * SLOT + SLOT, p.y);
    slot_store(out + (size_t)i * 4 * SLOT + 2 * SLOT, p.z); slot_store(out + (size_t)i * 4 * SLOT + 3 * SLOT, p.t);
#pragma unroll 1
    for (int k = 0; k < BITS; ++k) p = ge_double(p);
  }
}

}  // namespace d377
