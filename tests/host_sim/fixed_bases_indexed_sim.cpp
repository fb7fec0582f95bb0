// Test-only host build of d377_batch_fixed_msm_indexed's lane kernel (decaf377_amd/csrc/fixed_bases.hip): the combs of
// fixed_bases_sim.cpp, and over them the device's own indexed walk (curve.hpp: ge_fixed_msm_indexed_w8) with the kernel's
// term loader -- the index read once per term, the scalar reduced and halved, an absent term turned into scalar 0 on comb 0
// -- and the square-root-free compressor of the half point.  NOT part of the product: compiled by
// tests/test_fixed_bases_indexed_host.py with g++, it exists only under tests/.  It includes fixed_bases_sim.cpp, which
// includes sim.cpp, so fx_build / fx_msm (the dense walk) are here too and the two walks share one set of tables.
#include "fixed_bases_sim.cpp"

namespace {
// n sums of t terms, term p of sum i in comb idx[i t + p]; the lambda is k_fixed_msm_indexed_lane's, word for word
template <int BITS>
void run_indexed(const int* idx, const uint32_t* k, int t, size_t n, uint32_t* enc, uint32_t* xyzt_out) {
  const HostCombTabs<BITS> ft{g_fx.data()};
  const int m = g_fx_m;
  dcb_rounds<0>(n, enc, true,
    [&](HostDcbIO&, size_t, int) {},
    [&](HostDcbIO& io, size_t i, int j) {
      const size_t first = i * (size_t)t;
      const ge r = ge_fixed_msm_indexed_w8<BITS>(t, [&](int p, uint32_t kk[8]) -> int {
        const int b = idx[first + (size_t)p];
        memcpy(kk, k + 8 * (first + (size_t)p), 32);
        fr_reduce_words(kk);
        fr_half_words(kk);
        const uint32_t keep = (uint32_t)b < (uint32_t)m ? ~0u : 0u;
        for (int q = 0; q < 8; ++q) kk[q] &= keep;
        return (int)((uint32_t)b & keep);
      }, ft, DCB_WANT_T);
      if (xyzt_out) ge_store256(ge_double_fast(r, true), xyzt_out + 32 * i);
      dcb_put(io, j, ge_dcb_from_half(r, false));
    });
}
}  // namespace

extern "C" {
// idx: n x t indices (-1 = absent), k: n x t scalars (32 bytes each, any value), both term-major within a sum
int fx_msm_indexed(const int* idx, const uint32_t* k, int t, size_t n, uint32_t* enc, uint32_t* xyzt_out) {
  if (t < 1) return -1;
  if (g_fx_bits == 8) run_indexed<8>(idx, k, t, n, enc, xyzt_out);
  else if (g_fx_bits == 12) run_indexed<12>(idx, k, t, n, enc, xyzt_out);
  else return -1;
  return 0;
}
}
