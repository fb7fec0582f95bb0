// Test-only host build of d377_batch_msm_mixed's lane kernel (decaf377_amd/csrc/batch_msm_mixed.hip): the device's own per-sum
// body (mixed_sum.hpp: the Straus chain over the sum's variable points, the indexed comb walk over its registered bases, the
// addition that joins the two halves) with the kernel's two loaders, word for word, and the square-root-free compressor of the
// half point.  NOT part of the product: compiled by tests/test_msm_mixed_host.py with g++ (plain and with -DD377_BOUNDS) and
// included by the stand-alone program tests/cpp/msm_mixed.cpp; it exists only under tests/.  It includes
// fixed_bases_indexed_sim.cpp, which brings the combs (fx_build, fx_msm_indexed) and sim.cpp's Straus harness (sim_batch_msm).
#include "fixed_bases_indexed_sim.cpp"
#include "mixed_sum.hpp"

namespace {
// n sums: t fixed terms (idx, fk) and v variable terms (xyzt records, vk) each
template <int BITS>
void run_mixed(const int* idx, const uint32_t* fk, int t, const uint32_t* xyzt, const uint32_t* vk, int v, size_t n, uint32_t* enc,
               uint32_t* xyzt_out) {
  const HostCombTabs<BITS> ft{g_fx.data()};
  const int m = g_fx_m;
  dcb_rounds<0>(n, enc, true,
    [&](HostDcbIO&, size_t, int) {},
    [&](HostDcbIO& io, size_t i, int j) {
      HostStrausTab tab;
      const size_t vfirst = i * (size_t)v, ffirst = i * (size_t)t;
      const ge r = mixed_half_sum<BITS>(tab, v,
        [&](int p, uint32_t kk[8]) { memcpy(kk, vk + 8 * (vfirst + (size_t)p), 32); },
        [&](int p, ge* g) -> bool { *g = ge_load256(xyzt + 32 * (vfirst + (size_t)p)); return fe_is_zero(g->z); },
        t, [&](int p, uint32_t kk[8]) -> int {
          const int b = idx[ffirst + (size_t)p];
          memcpy(kk, fk + 8 * (ffirst + (size_t)p), 32);
          fr_reduce_words(kk);
          fr_half_words(kk);
          const uint32_t keep = (uint32_t)b < (uint32_t)m ? ~0u : 0u;
          for (int q = 0; q < 8; ++q) kk[q] &= keep;
          return (int)((uint32_t)b & keep);
        }, ft);
      if (xyzt_out) ge_store256(ge_double_fast(r, true), xyzt_out + 32 * i);
      dcb_put(io, j, ge_dcb_from_half(r, false));
    });
}
}  // namespace

extern "C" {
// over the combs of the last fx_build.  idx: n x t indices (-1 = absent), fk: n x t scalars, xyzt: n x v Element records,
// vk: n x v scalars (32 bytes each, any value); all term-major within a sum
int mx_msm_mixed(const int* idx, const uint32_t* fk, int t, const uint32_t* xyzt, const uint32_t* vk, int v, size_t n, uint32_t* enc,
                 uint32_t* xyzt_out) {
  if (t < 1 || v < 1 || v > 8) return -1;
  if (g_fx_bits == 8) run_mixed<8>(idx, fk, t, xyzt, vk, v, n, enc, xyzt_out);
  else if (g_fx_bits == 12) run_mixed<12>(idx, fk, t, xyzt, vk, v, n, enc, xyzt_out);
  else return -1;
  return 0;
}
// sim.cpp's sim_batch_msm (Encodings only) under a C name of this library's own, with the argument order of the call above
int mx_msm_small(const uint32_t* xyzt, const uint32_t* vk, int v, size_t n, uint32_t* enc) {
  if (v < 1 || v > 8) return -1;
  sim_batch_msm(xyzt, vk, v, n, enc);
  return 0;
}
}
