// batch_msm_mixed.hip -- many MIXED multiscalar sums at once (gfx950):
//     out[i] = sum_{j < t} fixed_scalar[i t + j] * B_{base_index[i t + j]}  +  sum_{p < v} var_scalar[i v + p] * P[i v + p]
// with the B registered as combs (d377_fixed_bases_create / _create_long) and 1 .. 8 variable points P per sum.
//
// The shapes: a signature or sigma-protocol check R' = s B - c A (one registered basepoint, one public key per signature;
// other curve libraries call it vartime_double_scalar_mul_basepoint), and a commitment with an opening v G_asset + r H + sum
// k_p P_p.  Composed of the existing calls such a sum is d377_batch_msm_small, d377_batch_fixed_msm_indexed, d377_batch_add
// and d377_batch_compress, with 128-byte Element records through host memory after each.  One lane can do all of it: both
// walks run on halved scalars and yield half their sum, the halves join in one unified addition, and one pass of the
// square-root-free compressor encodes the double (mixed_sum.hpp).
//
//   k_batch_msm_mixed_lane<BITS, ENCODED>   one lane per sum, built as batch_msm.hip's k_batch_msm_lane: chunks with one claimed
//                     lane set, the v window tables and the digit words of a lane in the per-device scratch area of the small
//                     sums (the same area), the sums of a chunk share one inversion per wave.  The fixed half gathers from the
//                     handle's combs with k_fixed_msm_indexed_lane's loader.
//
// There is no wave-per-sum route: the lane kernel takes every n, so a small batch is as long as one chain.
// d377_batch_msm_mixed[_encoded]_resident is the same launcher on device pointers and the caller's stream; it does not read the
// indices on the host and has fixed_bases.hip's k_index_verdict write one verdict record per call instead.
//
// A translation unit of its own, like batch_msm.hip: the register tables of the other units' kernels are measured artefacts.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>

#include "../../include/decaf377_amd.h"
#include "curve.hpp"
#include "device_util.hpp"
#include "dcb.hpp"
#include "straus.hpp"
#include "straus_tab.hpp"
#include "comb_tabs.hpp"
#include "mixed_sum.hpp"
#include "host_state.hpp"
#include "batch_host.hpp"

using namespace d377;

namespace {

constexpr int MX_VAR_MAX = D377_BATCH_MSM_MIXED_MAX_VAR;
constexpr int MX_FIXED_MAX = D377_FIXED_BASES_MAX;
static_assert(MX_VAR_MAX == D377_BATCH_MSM_MAX_TERMS && MX_VAR_MAX == 8, "a window's digits of the v points of a sum are the eight nibbles of one word");
static_assert(VB_ENTRIES == 9, "straus_sum stores entries 0 .. 8 of every point's table");

// One lane per sum.  The variable half is k_batch_msm_lane's body, the fixed half k_fixed_msm_indexed_lane's: an absent term
// (-1) walks scalar 0 on comb 0, and the unsigned compare treats every index outside 0 .. m-1 as absent, so no index can
// address past the m combs (the host form has refused those before the launch all the same; the resident form counts them
// in its verdict record, fixed_bases.hip: k_index_verdict).
template <int BITS, bool ENCODED>
__global__ void __launch_bounds__(BLOCK, WAVES_PER_SIMD)
k_batch_msm_mixed_lane(SqrtTables T, const uint32_t* tabs, const int* base_index, const uint8_t* fixed_scalar32, int m, int t,
                       const void* pts_in, const uint8_t* var_scalar32, int v, size_t n, uint8_t* out32, uint64_t* xyzt_out,
                       uint8_t* status, uint32_t* tab, uint32_t* dig, DcbScratch dcb) {
  __shared__ uint32_t lds_pow_[ENCODED ? POW_TAB * NL * BLOCK : 1];
  LdsPowTab pt;
  pt.col = lds_pow_ + (ENCODED ? threadIdx.x : 0);
  D377_DCB_BEGIN(out32);
  StrausTab st{tab, dig, (size_t)dcb.nslots * BLOCK, io.lane};
  const CombTabs<BITS> ft{tabs};
  dcb_rounds<0, true>(n, io, pt,
    [&](size_t, int) {},
    [&](size_t i, int j, const uint32_t (*)[8], bool) {
      const size_t vfirst = i * (size_t)v, ffirst = i * (size_t)t;
      const ge r = mixed_half_sum<BITS>(st, v,
        [&](int p, uint32_t k[8]) { load32(var_scalar32, vfirst + (size_t)p, k); },
        [&](int p, ge* g) -> bool {
          if (ENCODED) {
            uint32_t w[8];
            load32(reinterpret_cast<const uint8_t*>(pts_in), vfirst + (size_t)p, w);
            const uint32_t bad = ge_decompress(T, pt, w, g);
            status[vfirst + (size_t)p] = (uint8_t)bad;
            return bad != 0;
          }
          *g = load_ge_mont256(reinterpret_cast<const uint64_t*>(pts_in), vfirst + (size_t)p);
          D377_INVARIANT(T, *g, !fe_is_zero(g->z));
          return fe_is_zero(g->z);                                 // a record with Z = 0 is no group element: the identity
        },
        t, [&](int p, uint32_t k[8]) -> int {
          const int b = base_index[ffirst + (size_t)p];            // once per term
          load32(fixed_scalar32, ffirst + (size_t)p, k);
          fr_reduce_words(k);
          fr_half_words(k);
          const uint32_t keep = (uint32_t)b < (uint32_t)m ? ~0u : 0u;
#pragma unroll
          for (int q = 0; q < 8; ++q) k[q] &= keep;
          return (int)((uint32_t)b & keep);
        }, ft);
      D377_INVARIANT(T, r, true);
      if (xyzt_out) store_ge_mont256(xyzt_out, i, ge_double_fast(r, true));   // both walks ran on k / 2: the sum is the double
      dcb_put(io, j, ge_dcb_from_half(r, false));
    });
  D377_DCB_END();
}

// ------------------------------------------------------------------------------ host side ---
struct MixedArgs {
  const uint32_t* combs;       // the handle's combs on this device
  int m, bits;
  const int* index;            // n x t
  const uint8_t* fixed_scalars;
  size_t t;
  bool encoded;
  const void* pts_in;          // n x v records or Encodings
  const uint8_t* var_scalars;
  size_t v;
};

// everything on device pointers, enqueued on `s`; the caller holds ctx->mu
int mixed_launch(DeviceState& d, hipStream_t s, const MixedArgs& a, size_t n, uint8_t* out32, uint64_t* xyzt_out, uint8_t* status) {
  if (n == 0) return D377_OK;
  const SqrtTables T = d.tables();
  return with_width(a.bits, "batch_msm_mixed: the registration's comb width is none of 8, 12, 16, 18", [&](auto bb) -> int {
    constexpr int BITS = decltype(bb)::value;
    const void* fn = a.encoded ? reinterpret_cast<const void*>(k_batch_msm_mixed_lane<BITS, true>)
                               : reinterpret_cast<const void*>(k_batch_msm_mixed_lane<BITS, false>);
    int& lds = d.bmx_lds[a.encoded ? 1 : 0][width_slot(BITS)];
    int rc;
    if ((rc = lane_residency(fn, "k_batch_msm_mixed_lane", BITS, lds))) return rc;
    GuardScope vb{d.vb_guard, s};                            // the lane-set areas and the table scratch: queue behind their last user
    uint32_t *tab, *dig;
    if ((rc = straus_scratch_reserve(d, s, a.v,
           "batch_msm_mixed: the table scratch must grow, which cannot happen inside a stream capture",
           "batch_msm_mixed: hipMalloc of the table scratch failed (0.23 GB per variable term on 256 CUs)", &tab, &dig))) return rc;
    if ((rc = vb.acquire())) return rc;
    int grid;
    const DcbScratch dcb = lane_chunks(d, n, &grid);
    if (a.encoded)
      hipLaunchKernelGGL((k_batch_msm_mixed_lane<BITS, true>), dim3((unsigned)grid), dim3(BLOCK), lds, s, T, a.combs, a.index,
                         a.fixed_scalars, a.m, (int)a.t, a.pts_in, a.var_scalars, (int)a.v, n, out32, xyzt_out, status, tab, dig, dcb);
    else
      hipLaunchKernelGGL((k_batch_msm_mixed_lane<BITS, false>), dim3((unsigned)grid), dim3(BLOCK), lds, s, T, a.combs, a.index,
                         a.fixed_scalars, a.m, (int)a.t, a.pts_in, a.var_scalars, (int)a.v, n, out32, xyzt_out, status, tab, dig, dcb);
    HIP_TRY(hipGetLastError());
    return vb.finish();
  });
}

// one device's slice of a host batch: copies in, kernel, copies out, synchronised.  Staging: buf[0] the points, buf[1] the
// fixed scalars with the indices behind them (n t x 32 bytes: 16-byte aligned) and then the variable scalars, buf[2] the
// Encodings and then the Element records, buf[3] the status bytes.
int mixed_one(DeviceState& d, const FixedBases& fb, const uint32_t* combs, const int* index, const uint8_t* fixed_scalars, size_t t,
              bool encoded, const uint8_t* pts_in, const uint8_t* var_scalars, size_t v, size_t n, uint8_t* out32,
              uint64_t* xyzt_out, uint8_t* status) {
  if (n == 0) return D377_OK;
  return device_slice(d, [&]() -> int {
    const size_t rec = encoded ? 32 : 128, vterms = n * v, fterms = n * t;
    // fixed scalars | indices (padded to 16 bytes) | variable scalars
    const size_t idx_off = fterms * 32, var_off = idx_off + ((fterms * sizeof(int) + 15) & ~(size_t)15);
    int r;
    uint64_t* xyzt_dev;
    if ((r = ensure(d, 0, vterms * rec))) return r;
    if ((r = ensure(d, 1, var_off + vterms * 32))) return r;
    if ((r = sums_out_reserve(d, n, xyzt_out != nullptr, &xyzt_dev))) return r;
    if (encoded && (r = ensure(d, 3, vterms))) return r;
    HIP_TRY(hipMemcpyAsync(d.buf[0], pts_in, vterms * rec, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d.buf[1], fixed_scalars, fterms * 32, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d.buf[1] + idx_off, index, fterms * sizeof(int), hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d.buf[1] + var_off, var_scalars, vterms * 32, hipMemcpyHostToDevice, d.stream));
    const MixedArgs a{combs, (int)fb.m, fb.bits, reinterpret_cast<const int*>(d.buf[1] + idx_off), d.buf[1], t, encoded, d.buf[0],
                      d.buf[1] + var_off, v};
    if ((r = mixed_launch(d, d.stream, a, n, d.buf[2], xyzt_dev, d.buf[3]))) return r;
    if ((r = sums_out_copy(d, n, out32, xyzt_out))) return r;
    if (encoded) HIP_TRY(hipMemcpyAsync(status, d.buf[3], vterms, hipMemcpyDeviceToHost, d.stream));
    return D377_OK;
  });
}

// the checks both forms make first, before ctx is looked at: v, t, then null buffers when n > 0
int mixed_check(const char* who, const int* base_index, const uint8_t* fixed_scalar32, size_t t, bool encoded, const void* pts_in,
                const uint8_t* var_scalar32, size_t v, size_t n, const uint8_t* enc32_out, const uint8_t* status) {
  if (v < 1 || v > (size_t)MX_VAR_MAX)
    return fail(D377_ERR_ARG, "%s: v must be 1 .. 8 variable terms per sum (D377_BATCH_MSM_MIXED_MAX_VAR); d377_batch_fixed_msm_indexed serves v = 0", who);
  if (t < 1 || t > (size_t)MX_FIXED_MAX)
    return fail(D377_ERR_ARG, "%s: t must be 1 .. 64 fixed terms per sum (D377_FIXED_BASES_MAX); d377_batch_msm_small serves t = 0", who);
  if (n) {
    const char* null_arg = !base_index ? "base_index" : !fixed_scalar32 ? "fixed_scalar32" : !pts_in ? (encoded ? "enc32" : "xyzt")
                         : !var_scalar32 ? "var_scalar32" : !enc32_out ? "enc32_out" : (encoded && !status) ? "status" : nullptr;
    if (null_arg) {
      snprintf(d377_g_err, sizeof d377_g_err, "%s: %s is null", who, null_arg);
      return D377_ERR_ARG;
    }
  }
  return D377_OK;
}

// host pointers: every argument checked before any copy or launch, then contiguous slices of the SUMS over the context's
// devices (host_state.hpp: slice_over_devices)
int mixed_host(const char* who, d377_ctx* ctx, int64_t handle, const int* base_index, const uint8_t* fixed_scalar32, size_t t,
               bool encoded, const void* pts_in, const uint8_t* var_scalar32, size_t v, size_t n, uint8_t* enc32_out,
               uint64_t* xyzt_out, uint8_t* status) {
  if (int rc = mixed_check(who, base_index, fixed_scalar32, t, encoded, pts_in, var_scalar32, v, n, enc32_out, status)) return rc;
  if (!ctx) return fail(D377_ERR_ARG, "%s: ctx is null", who);
  std::lock_guard<std::mutex> lock(ctx->mu);
  const FixedBases* fb = fixed_bases_find(ctx, handle);
  if (!fb) return fail(D377_ERR_ARG, "%s: handle is not a live registration of this context", who);
  if (n > SIZE_MAX / 128 / (t > v ? t : v)) return fail(D377_ERR_ARG, "%s: n x t or n x v overflows", who);
  // every index, before any copy or launch: no kernel sees one it could read out of bounds with
  const size_t fterms = n * t;
  const int m = (int)fb->m;
  for (size_t p = 0; p < fterms; ++p) {
    const int b = base_index[p];
    if (b < -1 || b >= m) {
      snprintf(d377_g_err, sizeof d377_g_err,
               "%s: base_index[%zu] = %d (sum %zu, term %zu) is neither -1 nor a base 0 .. %d of this registration",
               who, p, b, p / t, p % t, m - 1);
      return D377_ERR_ARG;
    }
  }
  if (n == 0) return D377_OK;
  const size_t rec = encoded ? 32 : 128;
  const uint8_t* pts = reinterpret_cast<const uint8_t*>(pts_in);
  return slice_over_devices(ctx, n, [&](size_t k, size_t lo, size_t cnt) {
    return mixed_one(ctx->devs[k], *fb, fb->tab[k], base_index + lo * t, fixed_scalar32 + lo * t * 32, t, encoded, pts + lo * v * rec,
                     var_scalar32 + lo * v * 32, v, cnt, enc32_out + lo * 32, xyzt_out ? xyzt_out + lo * 16 : nullptr,
                     encoded ? status + lo * v : nullptr);
  });
}

// device pointers: mixed_host's checks in its order up to the handle -- then dev, the handle and alignment instead of the walk
// over the indices, which the verdict kernel makes on the device in front of the sums kernel (index_verdict.hpp)
int mixed_resident(const char* who, d377_ctx* ctx, int dev, void* stream, int64_t handle, const int* base_index,
                   const uint8_t* fixed_scalar32, size_t t, bool encoded, const void* pts_in, const uint8_t* var_scalar32, size_t v,
                   size_t n, uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status, uint64_t* verdict) {
  if (int rc = mixed_check(who, base_index, fixed_scalar32, t, encoded, pts_in, var_scalar32, v, n, enc32_out, status)) return rc;
  if (!ctx) return fail(D377_ERR_ARG, "%s: ctx is null", who);
  std::lock_guard<std::mutex> lock(ctx->mu);
  ResidentCall c;
  const void* rec[5] = {fixed_scalar32, pts_in, var_scalar32, enc32_out, xyzt_out};
  int rc;
  if ((rc = resident_enter(who, ctx, dev, handle, rec, 5, base_index, verdict, &c))) return rc;
  if (n > SIZE_MAX / 128 / (t > v ? t : v)) return fail(D377_ERR_ARG, "%s: n x t or n x v overflows", who);
  if (n == 0) return D377_OK;
  if (verdict && (rc = index_verdict_launch(*c.d, (hipStream_t)stream, base_index, n * t, (int)c.fb->m, verdict))) return rc;
  const MixedArgs a{c.tab, (int)c.fb->m, c.fb->bits, base_index, fixed_scalar32, t, encoded, pts_in, var_scalar32, v};
  return mixed_launch(*c.d, (hipStream_t)stream, a, n, enc32_out, xyzt_out, status);
}

}  // namespace

extern "C" {

int d377_batch_msm_mixed_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const int* base_index,
                                  const uint8_t* fixed_scalar32, size_t t, const uint64_t* xyzt, const uint8_t* var_scalar32, size_t v,
                                  size_t n, uint8_t* enc32_out, uint64_t* xyzt_out, uint64_t* verdict) {
  return mixed_resident("d377_batch_msm_mixed_resident", ctx, dev, stream, handle, base_index, fixed_scalar32, t, false, xyzt,
                        var_scalar32, v, n, enc32_out, xyzt_out, nullptr, verdict);
}
int d377_batch_msm_mixed_encoded_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const int* base_index,
                                          const uint8_t* fixed_scalar32, size_t t, const uint8_t* enc32, const uint8_t* var_scalar32,
                                          size_t v, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status,
                                          uint64_t* verdict) {
  return mixed_resident("d377_batch_msm_mixed_encoded_resident", ctx, dev, stream, handle, base_index, fixed_scalar32, t, true,
                        enc32, var_scalar32, v, n, enc32_out, xyzt_out, status, verdict);
}

int d377_batch_msm_mixed(d377_ctx* ctx, int64_t handle, const int* base_index, const uint8_t* fixed_scalar32, size_t t,
                         const uint64_t* xyzt, const uint8_t* var_scalar32, size_t v, size_t n, uint8_t* enc32_out,
                         uint64_t* xyzt_out) {
  return mixed_host("d377_batch_msm_mixed", ctx, handle, base_index, fixed_scalar32, t, false, xyzt, var_scalar32, v, n, enc32_out,
                    xyzt_out, nullptr);
}
int d377_batch_msm_mixed_encoded(d377_ctx* ctx, int64_t handle, const int* base_index, const uint8_t* fixed_scalar32, size_t t,
                                 const uint8_t* enc32, const uint8_t* var_scalar32, size_t v, size_t n, uint8_t* enc32_out,
                                 uint64_t* xyzt_out, uint8_t* status) {
  return mixed_host("d377_batch_msm_mixed_encoded", ctx, handle, base_index, fixed_scalar32, t, true, enc32, var_scalar32, v, n,
                    enc32_out, xyzt_out, status);
}

}  // extern "C"
