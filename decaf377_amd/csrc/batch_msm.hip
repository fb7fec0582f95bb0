// batch_msm.hip -- many SMALL multiscalar sums at once (gfx950): out[i] = sum_{j < m} scalar[i m + j] * point[i m + j], m = 1 .. 8.
//
// The reference's Element::vartime_multiscalar_mul (src/ark_curve/element/projective.rs:99-117) is a fold of `acc + scalar *
// point`, and the shape its own test exercises is a 3-term sum per case (tests/operations.rs:44-60).  d377_msm (msm.hip) is ONE
// sum per call -- Pippenger, with a floor of a quarter of a millisecond -- so a caller with 2^16 independent 3-term sums had to
// compose three scalar-multiplication batches and two addition batches.  Here every sum is one Straus chain: the m points of a
// sum share ONE chain of 252 doublings, each window adds one entry of each point's table of cached 0 .. 8 P (signed 4-bit
// digits of k / 2 mod r, the encoding of the double needs no square root: curve.hpp).  63 x 4 doublings + 64 m additions + the
// m tables, against m x (63 x 4 doublings + 63 additions + a table): 0.51 of the composition's instructions at m = 3.
//
//   k_batch_msm_lane   one lane per sum, in chunks like k_scalar_mul_var (dcb.hpp): the m tables of a lane and its digit words
//                      live in a per-device scratch area that exists once per resident lane (m x 1 728 + 256 bytes per lane,
//                      grown on first use), the sums of a chunk share one inversion per wave
//   k_batch_msm_wave   one WAVE per sum in the lane-spread form (row_ops.hpp), tables in LDS: batches up to one sum per SIMD,
//                      where a call is as long as one chain
//
// A translation unit of its own, like codec_chunked.hip: the register tables of d377.hip's kernels are measured artefacts.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/decaf377_amd.h"
#include "curve.hpp"
#include "device_util.hpp"
#include "dcb.hpp"
#include "quad_ops.hpp"
#include "row_ops.hpp"
#include "straus.hpp"
#include "straus_tab.hpp"
#include "host_state.hpp"
#include "batch_host.hpp"

using namespace d377;

namespace {

constexpr int BM_MAX = D377_BATCH_MSM_MAX_TERMS;
static_assert(BM_MAX == 8, "a window's digits of the m points of a sum are the eight nibbles of one word");
static_assert(VB_ENTRIES == 9, "straus_sum stores entries 0 .. 8 of every point's table");

// One lane per sum; its tables and digit words are the per-lane scratch of straus_tab.hpp.
// The point loader below (the `[&](int p, ge* g) -> bool` lambda) has two copies, in k_msm_long_lane and
// k_batch_msm_mixed_lane.  It is not shared: behind a __forceinline__ function template, by reference, by value or as a
// functor, the register allocation of this kernel moves -- k_batch_msm_lane<true> 692 -> 696 bytes of scratch and 9 more
// instructions, k_batch_msm_lane<false> renumbered throughout -- and nobody can measure one more spill here.
template <bool ENCODED>
__global__ void __launch_bounds__(BLOCK, WAVES_PER_SIMD)
k_batch_msm_lane(SqrtTables T, const void* pts_in, const uint8_t* scalar32, int m, size_t n, uint8_t* out32, uint64_t* xyzt_out,
                 uint8_t* status, uint32_t* tab, uint32_t* dig, DcbScratch dcb) {
  __shared__ uint32_t lds_pow_[ENCODED ? POW_TAB * NL * BLOCK : 1];
  LdsPowTab pt;
  pt.col = lds_pow_ + (ENCODED ? threadIdx.x : 0);
  D377_DCB_BEGIN(out32);
  StrausTab st{tab, dig, (size_t)dcb.nslots * BLOCK, io.lane};
  dcb_rounds<0, true>(n, io, pt,
    [&](size_t, int) {},
    [&](size_t i, int j, const uint32_t (*)[8], bool) {
      const size_t first = i * (size_t)m;
      const ge r = straus_sum(st, m, [&](int p, uint32_t k[8]) { load32(scalar32, first + (size_t)p, k); }, [&](int p, ge* g) -> bool {
        if (ENCODED) {
          uint32_t w[8];
          load32(reinterpret_cast<const uint8_t*>(pts_in), first + (size_t)p, w);
          const uint32_t bad = ge_decompress(T, pt, w, g);
          status[first + (size_t)p] = (uint8_t)bad;
          return bad != 0;
        }
        *g = load_ge_mont256(reinterpret_cast<const uint64_t*>(pts_in), first + (size_t)p);
        D377_INVARIANT(T, *g, !fe_is_zero(g->z));
        return fe_is_zero(g->z);                                   // a record with Z = 0 is no group element: the identity
      }, DCB_WANT_T);
      if (xyzt_out) store_ge_mont256(xyzt_out, i, ge_double_fast(r, true));   // the chain ran on k / 2: the sum is the double
      dcb_put(io, j, ge_dcb_from_half(r, false));
    });
  D377_DCB_END();
}

// ---- one wave per sum: straus_tab.hpp's chain, then the Element record and the compressor for a single element ----------------
struct OneIO {                                                   // the square-root-free compressor's records for a single element
  uint32_t st[4][8], parked_[8], out[8];
  __device__ __forceinline__ void put(int s, int, const uint32_t* w) { for (int k = 0; k < 8; ++k) st[s][k] = w[k]; }
  __device__ __forceinline__ void get(int s, int, uint32_t* w) const { for (int k = 0; k < 8; ++k) w[k] = st[s][k]; }
  __device__ __forceinline__ void park(int, const uint32_t* w) { for (int k = 0; k < 8; ++k) parked_[k] = w[k]; }
  __device__ __forceinline__ void parked(int, uint32_t* w) const { for (int k = 0; k < 8; ++k) w[k] = parked_[k]; }
  __device__ __forceinline__ void emit(int, const uint32_t* w) { for (int k = 0; k < 8; ++k) out[k] = w[k]; }
};
using row::RQ_WORDS;
template <bool ENCODED>
__global__ void __launch_bounds__(64)
k_batch_msm_wave(SqrtTables T, const void* pts_in, const uint8_t* scalar32, int m, size_t n, uint8_t* out32, uint64_t* xyzt_out,
                 uint8_t* status) {
  extern __shared__ uint32_t tab[];                                // m tables of RQ_TAB_ENTRIES x RQ_WORDS words (dynamic: 2 304 bytes per term)
  __shared__ uint32_t xrec[2 * RQ_WORDS];
  __shared__ uint32_t sdg[BM_MAX][8];                              // the points' signed digits (wave-uniform reads in the loop)
  const int t = threadIdx.x;
  (void)n;                                                         // grid = n
  const ge r = straus_wave_sum<ENCODED>(T, pts_in, scalar32, (size_t)blockIdx.x * (size_t)m, m, status, tab, xrec, sdg);
  if (xyzt_out && t == 0) store_ge_mont256(xyzt_out, blockIdx.x, ge_double_fast(r, true));
  OneIO io;
  dcb_put(io, 0, ge_dcb_from_half(r, false));
  dcb_finish_with(io, 1, [](const fe& c) { return row::fe_invert_wave(c); });   // (every lane holds the same element)
  if (t == 0) store32(out32, blockIdx.x, io.out);
}

// ------------------------------------------------------------------------------ host side ---
// everything on device pointers, enqueued on `s`; the caller holds ctx->mu
int batch_msm_launch(DeviceState& d, hipStream_t s, bool encoded, const void* pts_in, const uint8_t* scalars, size_t m, size_t n,
                     uint8_t* out32, uint64_t* xyzt_out, uint8_t* status) {
  if (n == 0) return D377_OK;
  const SqrtTables T = d.tables();
  if (n <= sums_wave_max(d)) {                               // up to four sums per SIMD: a wave per sum (launch_plan.hpp)
    const size_t lds = m * row::RQ_TAB_ENTRIES * RQ_WORDS * sizeof(uint32_t);
    if (encoded) hipLaunchKernelGGL(k_batch_msm_wave<true>, dim3((unsigned)n), dim3(64), lds, s, T, pts_in, scalars, (int)m, n, out32, xyzt_out, status);
    else hipLaunchKernelGGL(k_batch_msm_wave<false>, dim3((unsigned)n), dim3(64), lds, s, T, pts_in, scalars, (int)m, n, out32, xyzt_out, status);
    HIP_TRY(hipGetLastError());
    return D377_OK;
  }
  const void* fn = encoded ? reinterpret_cast<const void*>(k_batch_msm_lane<true>) : reinterpret_cast<const void*>(k_batch_msm_lane<false>);
  int& lds = d.bm_lds[encoded ? 1 : 0];
  int rc;
  if ((rc = lane_residency(fn, "k_batch_msm_lane", encoded, lds))) return rc;
  GuardScope vb{d.vb_guard, s};                              // the lane-set areas and the table scratch: queue behind their last user
  uint32_t *tab, *dig;
  if ((rc = straus_scratch_reserve(d, s, m,
         "batch_msm_small: the table scratch must grow, which cannot happen inside a stream capture -- run one call with this many terms first",
         "batch_msm_small: hipMalloc of the table scratch failed (0.23 GB per term on 256 CUs)", &tab, &dig))) return rc;
  if ((rc = vb.acquire())) return rc;
  int grid;
  const DcbScratch dcb = lane_chunks(d, n, &grid);
  if (encoded)
    hipLaunchKernelGGL(k_batch_msm_lane<true>, dim3((unsigned)grid), dim3(BLOCK), lds, s, T, pts_in, scalars, (int)m, n, out32, xyzt_out, status, tab, dig, dcb);
  else
    hipLaunchKernelGGL(k_batch_msm_lane<false>, dim3((unsigned)grid), dim3(BLOCK), lds, s, T, pts_in, scalars, (int)m, n, out32, xyzt_out, status, tab, dig, dcb);
  HIP_TRY(hipGetLastError());
  return vb.finish();
}

int check_terms(size_t m) {
  if (m < 1 || m > (size_t)BM_MAX) return fail(D377_ERR_ARG, "%s", "batch_msm_small: 1 .. 8 terms per sum (D377_BATCH_MSM_MAX_TERMS); d377_msm for one long sum");
  return D377_OK;
}

// one device's slice of a host batch: copies in, kernel, copies out, synchronised
int batch_msm_one(DeviceState& d, bool encoded, const uint8_t* pts_in, const uint8_t* scalars, size_t m, size_t n, uint8_t* out32,
                  uint64_t* xyzt_out, uint8_t* status) {
  if (n == 0) return D377_OK;
  return device_slice(d, [&]() -> int {
    const size_t rec = encoded ? 32 : 128, terms = n * m;
    int r;
    uint64_t* xyzt_dev;
    if ((r = ensure(d, 0, terms * rec))) return r;
    if ((r = ensure(d, 1, terms * 32))) return r;
    if ((r = sums_out_reserve(d, n, xyzt_out != nullptr, &xyzt_dev))) return r;
    if (encoded && (r = ensure(d, 3, terms))) return r;
    HIP_TRY(hipMemcpyAsync(d.buf[0], pts_in, terms * rec, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d.buf[1], scalars, terms * 32, hipMemcpyHostToDevice, d.stream));
    if ((r = batch_msm_launch(d, d.stream, encoded, d.buf[0], d.buf[1], m, n, d.buf[2], xyzt_dev, d.buf[3]))) return r;
    if ((r = sums_out_copy(d, n, out32, xyzt_out))) return r;
    if (encoded) HIP_TRY(hipMemcpyAsync(status, d.buf[3], terms, hipMemcpyDeviceToHost, d.stream));
    return D377_OK;
  });
}

// host pointers: contiguous slices of the SUMS over the context's devices (host_state.hpp: slice_over_devices)
int batch_msm_host(d377_ctx* ctx, bool encoded, const void* pts_in, const uint8_t* scalars, size_t m, size_t n, uint8_t* out32,
                   uint64_t* xyzt_out, uint8_t* status) {
  if (!ctx) return fail(D377_ERR_ARG, "%s", "null context");
  int rc = check_terms(m);
  if (rc) return rc;
  if (n && (!pts_in || !scalars || !out32 || (encoded && !status))) return fail(D377_ERR_ARG, "%s", "null buffer");
  if (n == 0) return D377_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t rec = encoded ? 32 : 128;
  return slice_over_devices(ctx, n, [&](size_t k, size_t lo, size_t cnt) {
    return batch_msm_one(ctx->devs[k], encoded, (const uint8_t*)pts_in + lo * m * rec, scalars + lo * m * 32, m, cnt, out32 + lo * 32,
                         xyzt_out ? xyzt_out + lo * 16 : nullptr, encoded ? status + lo * m : nullptr);
  });
}

int batch_msm_dev(d377_ctx* ctx, int dev, void* stream, bool encoded, const void* pts_in, const uint8_t* scalars, size_t m, size_t n,
                  uint8_t* out32, uint64_t* xyzt_out, uint8_t* status) {
  if (!ctx) return fail(D377_ERR_ARG, "%s", "null context");
  if (dev < 0 || (size_t)dev >= ctx->devs.size()) return fail(D377_ERR_ARG, "%s", "device index out of range");
  int rc = check_terms(m);
  if (rc) return rc;
  if (n && (!pts_in || !scalars || !out32 || (encoded && !status))) return fail(D377_ERR_ARG, "%s", "null buffer");
  if (!aligned16(pts_in) || !aligned16(scalars) || !aligned16(out32) || !aligned16(xyzt_out))
    return fail(D377_ERR_ARG, "%s", "device record buffers must be 16-byte aligned");
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceState& d = ctx->devs[(size_t)dev];
  HIP_TRY(hipSetDevice(d.id));
  return batch_msm_launch(d, (hipStream_t)stream, encoded, pts_in, scalars, m, n, out32, xyzt_out, status);
}

}  // namespace

extern "C" {

int d377_batch_msm_small(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalar32, size_t m, size_t n, uint8_t* enc32_out,
                         uint64_t* xyzt_out) {
  return batch_msm_host(ctx, false, xyzt, scalar32, m, n, enc32_out, xyzt_out, nullptr);
}
int d377_batch_msm_small_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, size_t m, size_t n, uint8_t* enc32_out,
                                 uint64_t* xyzt_out, uint8_t* status) {
  return batch_msm_host(ctx, true, enc32, scalar32, m, n, enc32_out, xyzt_out, status);
}
int d377_batch_msm_small_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalar32, size_t m, size_t n,
                             uint8_t* enc32_out, uint64_t* xyzt_out) {
  return batch_msm_dev(ctx, dev, stream, false, xyzt, scalar32, m, n, enc32_out, xyzt_out, nullptr);
}
int d377_batch_msm_small_encoded_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalar32, size_t m,
                                     size_t n, uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status) {
  return batch_msm_dev(ctx, dev, stream, true, enc32, scalar32, m, n, enc32_out, xyzt_out, status);
}

}  // extern "C"
