// Test-only host build of d377_batch_fixed_msm's lane kernel (decaf377_amd/csrc/fixed_bases.hip): combs of caller-chosen
// bases built on the host, the device's own multi-comb walk (curve.hpp: ge_fixed_msm_w8) over them with the halved scalars,
// and the square-root-free compressor of the half point -- so the walk can be checked against the oracle on a machine
// with no GPU.  NOT part of the product: compiled by tests/test_fixed_bases_host.py with g++, it exists only under tests/.
// It reuses sim.cpp's host harness (the round structure of dcb_rounds, the record I/O), which it includes.
#include "sim.cpp"

namespace {
// the combs of m bases, back to back as on the device (fixed_comb.hpp): entry c of window i of base j, 27 limbs per record
std::vector<uint32_t> g_fx;
int g_fx_bits = 0, g_fx_m = 0;

template <int BITS>
struct HostCombTabs {
  const uint32_t* p;
  gea load(int j, int i, int c, bool swap) const {
    gea g;
    const uint32_t* q = p + (((size_t)j * FbShape<BITS>::windows + i) * FbShape<BITS>::entries + c) * 27;
    for (int k = 0; k < 9; ++k) { g.ypx.l[k] = q[(swap ? 9 : 0) + k]; g.ymx.l[k] = q[(swap ? 0 : 9) + k]; g.kt.l[k] = q[18 + k]; }
    fe_assume_carried(g.ypx, 26.0); fe_assume_carried(g.ymx, 26.0); fe_assume_carried(g.kt, 9.0);
    return g;
  }
};

// window i of base j holds c * 2^(BITS i) * B_j in affine cached form (the k_fb_window_bases + k_init_fbase construction,
// one inversion per entry instead of one per run: the records' values are the same)
template <int BITS>
void build(const uint32_t* xyzt, int m) {
  using Sh = FbShape<BITS>;
  g_fx.assign((size_t)m * Sh::windows * Sh::entries * 27, 0);
  for (int j = 0; j < m; ++j) {
    ge pi = ge_load256(xyzt + 32 * j);
    if (fe_is_zero(pi.z)) pi = ge_identity();                 // a record with Z = 0 counts as the identity
    for (int i = 0; i < Sh::windows; ++i) {
      ge acc = ge_identity();
      for (int c = 0; c < Sh::entries; ++c) {
        const fe zi = fe_invert(acc.z);
        const gea r = gea_from_affine(fe_mul(acc.x, zi), fe_mul(acc.y, zi));
        uint32_t* q = g_fx.data() + (((size_t)j * Sh::windows + i) * Sh::entries + c) * 27;
        for (int k = 0; k < 9; ++k) { q[k] = r.ypx.l[k]; q[9 + k] = r.ymx.l[k]; q[18 + k] = r.kt.l[k]; }
        acc = ge_add(acc, pi);
      }
      for (int b = 0; b < BITS; ++b) pi = ge_double(pi);
    }
  }
}

// n sums over the registered bases: the encodings through the halved walk and the compressor, as the lane kernel does;
// xyzt_out (if given): the sums as records, 2 H as the kernel writes them
template <int BITS>
void run(const uint32_t* k, size_t n, uint32_t* enc, uint32_t* xyzt_out) {
  const HostCombTabs<BITS> ft{g_fx.data()};
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
}  // namespace

extern "C" {
// bases: m Element records (16 u64 = 32 u32 each); bits: 8 or 12 -> 0, or -1 for another width
int fx_build(const uint32_t* xyzt, int m, int bits) {
  g_fx_m = m;
  g_fx_bits = bits;
  if (bits == 8) build<8>(xyzt, m);
  else if (bits == 12) build<12>(xyzt, m);
  else return -1;
  return 0;
}
// k: n x m scalars (32 bytes each, any value), term-major within a sum
int fx_msm(const uint32_t* k, size_t n, uint32_t* enc, uint32_t* xyzt_out) {
  if (g_fx_bits == 8) run<8>(k, n, enc, xyzt_out);
  else if (g_fx_bits == 12) run<12>(k, n, enc, xyzt_out);
  else return -1;
  return 0;
}
}
