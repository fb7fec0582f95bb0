// batch_msm_long.hip -- many multiscalar sums of 9 .. 4096 terms each (gfx950): out[i] = sum_{j < m} scalar[i m + j] * point[i m + j].
//
// Between d377_msm (ONE sum per call, Pippenger, a floor of a quarter of a millisecond) and d377_batch_msm_small (n sums of at
// most 8 terms) a caller with a thousand sums of a few hundred terms had to call one n times or compose the other with rounds
// of additions through host memory.  Here every sum is cut into g = ceil(m / 8) groups of b = ceil(m / g) terms
// (batch_msm_long_plan.hpp), every group is the Straus chain of the small sums (straus.hpp, unchanged), and the g partial
// sums of a sum are folded on the device:
//
//   k_msm_long_lane   one lane per PARTIAL sum, in chunks with the per-lane table scratch of batch_msm.hip's lane kernel (the
//                     same area, b <= 8 tables per lane); every chain of a launch runs b slots, the slots of a sum's last
//                     group that lie past its end are dead and read nothing
//   k_msm_long_wave   one wave per partial sum in the lane-spread form (row_ops.hpp), tables in LDS: calls of up to four
//                     partial sums per SIMD (one sum of 4096 terms is 512 of them)
//   k_msm_long_fold   one lane adds up to BML_FOLD = 16 consecutive partial sums of one sum (the full addition of k_add on
//                     records, no conversion); repeated until one record per sum is left -- three levels at g = 512
//
// The chains write their partial sums as Element records (the double of the chain's result, as xyzt_out of the small sums)
// and skip the compressor; the last fold level's records go through the chunked compressor with batched inversions
// (codec_chunked.hip).  Everything below the host copy layer works on device pointers and a stream, and
// d377_batch_long_msm[_encoded]_resident (include/decaf377_amd_long_sums.h) are that launch on the caller's buffers.
//
// A translation unit of its own, like batch_msm.hip: the register tables of the other units' kernels are measured artefacts.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
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
#include "codec_chunked.hpp"
#include "batch_msm_long_plan.hpp"
#include "msm_long_fold.hpp"

using namespace d377;

namespace {

constexpr size_t BML_MAX = D377_BATCH_MSM_LONG_MAX_TERMS;
static_assert(BML_GROUP_MAX == D377_BATCH_MSM_MAX_TERMS, "a group is one chain of the small sums");
static_assert(VB_ENTRIES == 9, "straus_sum stores entries 0 .. 8 of every point's table");

// ---- one lane per partial sum -----------------------------------------------------------------------------------------------
// np = n g partial sums; partial p = s g + q reads the terms from s m + q b.  status: one byte per TERM, written for live slots only.
template <bool ENCODED>
__global__ void __launch_bounds__(BLOCK, WAVES_PER_SIMD)
k_msm_long_lane(SqrtTables T, const void* pts_in, const uint8_t* scalar32, LongPlan plan, size_t np, uint64_t* partials,
                uint8_t* status, uint32_t* tab, uint32_t* dig, DcbScratch dcb) {
  __shared__ uint32_t lds_pow_[ENCODED ? POW_TAB * NL * BLOCK : 1];
  LdsPowTab pt;
  pt.col = lds_pow_ + (ENCODED ? threadIdx.x : 0);
  D377_DCB_BEGIN(partials);                                  // (no compressor here: the chunk walk never writes through io.out32)
  StrausTab st{tab, dig, (size_t)dcb.nslots * BLOCK, io.lane};
  dcb_rounds<0, false>(np, io, pt,
    [&](size_t, int) {},
    [&](size_t i, int, const uint32_t (*)[8], bool) {
      const size_t s = i / plan.g, q = i % plan.g;
      const size_t first = s * plan.m + plan.first(q);
      const int live = (int)plan.count(q);                   // 1 .. b; the slots from `live` on are past the end of the sum
      const ge r = straus_sum(st, (int)plan.b, [&](int p, uint32_t k[8]) {
        if (p < live) { load32(scalar32, first + (size_t)p, k); return; }
#pragma unroll
        for (int w = 0; w < 8; ++w) k[w] = 0;                 // a dead slot: no scalar read
      }, [&](int p, ge* g) -> bool {
        if (p >= live) { *g = ge_identity(); return true; }   // a dead slot: no point read, no status write
        if (ENCODED) {
          uint32_t w[8];
          load32(reinterpret_cast<const uint8_t*>(pts_in), first + (size_t)p, w);
          const uint32_t bad = ge_decompress(T, pt, w, g);
          status[first + (size_t)p] = (uint8_t)bad;
          return bad != 0;
        }
        *g = load_ge_mont256(reinterpret_cast<const uint64_t*>(pts_in), first + (size_t)p);
        D377_INVARIANT(T, *g, !fe_is_zero(g->z));
        return fe_is_zero(g->z);                              // a record with Z = 0 is no group element: the identity
      }, DCB_WANT_T);
      store_ge_mont256(partials, i, ge_double_fast(r, true)); // the chain ran on k / 2: the partial sum is the double
    });
  D377_DCB_END();
}

// ---- one wave per partial sum: straus_tab.hpp's chain on a group, without the compressor --------------------------------------
// The chain's term count is uniform over the workgroup, so the wave form runs the group's live terms only: it has no dead slots.
using row::RQ_WORDS;
template <bool ENCODED>
__global__ void __launch_bounds__(64)
k_msm_long_wave(SqrtTables T, const void* pts_in, const uint8_t* scalar32, LongPlan plan, size_t np, uint64_t* partials,
                uint8_t* status) {
  extern __shared__ uint32_t tab[];                                // b tables of RQ_TAB_ENTRIES x RQ_WORDS words (dynamic: 2 304 bytes per term)
  __shared__ uint32_t xrec[2 * RQ_WORDS];
  __shared__ uint32_t sdg[BML_GROUP_MAX][8];                       // the points' signed digits (wave-uniform reads in the loop)
  const size_t part = blockIdx.x;                                  // grid = np
  if (part >= np) return;
  const size_t gq = part % plan.g;
  const ge r = straus_wave_sum<ENCODED>(T, pts_in, scalar32, (part / plan.g) * plan.m + plan.first(gq), (int)plan.count(gq), status,
                                        tab, xrec, sdg);
  if (threadIdx.x == 0) store_ge_mont256(partials, part, ge_double_fast(r, true));
}

// ---- the fold: c records per sum -> ceil(c / BML_FOLD) ------------------------------------------------------------------------
// Lane L = s oc + f adds the records [f BML_FOLD, f BML_FOLD + fold_count) of sum s with k_add's full addition on the records as
// they lie in memory (curve.hpp, "records used without conversion") and writes record L of the next level.  A lane's records
// are consecutive: 2 KiB per lane.  Lanes past the end of the level do nothing; a sum's last lane may add fewer records.
__global__ void __launch_bounds__(BLOCK) k_msm_long_fold(const uint64_t* in, size_t c, size_t nsums, uint64_t* out) {
  const size_t oc = fold_out(c), total = nsums * oc;
  for (size_t L = (size_t)blockIdx.x * BLOCK + threadIdx.x; L < total; L += (size_t)gridDim.x * BLOCK) {
    const size_t s = L / oc, f = L % oc;
    const size_t lo = s * c + f * BML_FOLD;
    const int cnt = (int)fold_count(c, f);
    uint32_t acc[32];
    load_record128(in, lo, acc);
#pragma unroll 1
    for (int j = 1; j < cnt; ++j) {
      uint32_t q[32], r[32];
      load_record128(in, lo + (size_t)j, q);
      ge_add_raw_words(acc, q, false, r);
#pragma unroll
      for (int w = 0; w < 32; ++w) acc[w] = r[w];
    }
    store_record128(out, L, acc);
  }
}

// ------------------------------------------------------------------------------ host side ---
int fail_size(int code, const char* fmt, size_t a) {
  char msg[256];
  snprintf(msg, sizeof msg, fmt, a);
  return fail(code, "%s", msg);
}

// records the area must hold for n sums of g partial sums: the partial sums, then the two halves the fold levels alternate between
size_t partial_records(size_t n, size_t g) { return n * g + 2 * n * fold_out(g); }

}  // namespace

// ---- what both this unit's chains and fixed_bases.hip's segments end in (msm_long_fold.hpp) ----------------------------------
namespace d377 {

int long_sums_partials(DeviceState& d, hipStream_t s, size_t n, size_t g, uint64_t** partials) {
  *partials = nullptr;
  int rc;
  if ((rc = d.bml_partials.reserve(d.vb_guard, s, partial_records(n, g) * 128, SLACK_PARTIALS,
         "batch_msm_long: the partial sums' area must grow, which cannot happen inside a stream capture",
         "batch_msm_long: hipMalloc of the partial sums' area failed (%zu bytes: 128 bytes per group of up to 8 terms)"))) return rc;
  *partials = d.bml_partials.as<uint64_t>();
  return D377_OK;
}

int long_sums_partials_records(DeviceState& d, hipStream_t s, size_t records, size_t tail_bytes, uint64_t** partials) {
  *partials = nullptr;
  int rc;
  if ((rc = d.bml_partials.reserve(d.vb_guard, s, records * 128 + tail_bytes, SLACK_PARTIALS,
         "batch_segmented_msm: the partial sums' area must grow, which cannot happen inside a stream capture",
         "batch_segmented_msm: hipMalloc of the partial sums' area failed (%zu bytes: 128 bytes per slot of a chain or a fold level)"))) return rc;
  *partials = d.bml_partials.as<uint64_t>();
  return D377_OK;
}

int long_sums_fold_compress(DeviceState& d, hipStream_t s, size_t n, size_t g, uint8_t* out32, uint64_t* xyzt_out) {
  uint64_t* partials = d.bml_partials.as<uint64_t>();
  const size_t np = n * g;
  uint64_t* half[2] = {partials + np * 16, partials + (np + n * fold_out(g)) * 16};

  // ---- fold levels until one record per sum is left; the last level writes the caller's Element records if asked
  const uint64_t* cur = partials;
  int turn = 0;
  for (size_t c = g; c > 1; c = fold_out(c)) {
    const size_t oc = fold_out(c), lanes = n * oc;
    uint64_t* dst = (oc == 1 && xyzt_out) ? xyzt_out : half[turn];
    hipLaunchKernelGGL(k_msm_long_fold, dim3((unsigned)fold_grid(d, lanes)), dim3(BLOCK), 0, s, cur, c, n, dst);
    HIP_TRY(hipGetLastError());
    cur = dst;
    turn ^= 1;
  }

  // ---- the sums' Encodings, in chunks with batched inversions (codec_chunked.hip)
  int grid;
  const DcbScratch dcb = lane_chunks(d, n, &grid);
  return codec_chunked_launch(d, s, false, cur, n, out32, nullptr, grid, dcb);
}

}  // namespace d377

namespace {

// everything on device pointers, enqueued on `s`; the caller holds ctx->mu.  m > 8.
int batch_msm_long_launch(DeviceState& d, hipStream_t s, bool encoded, const void* pts_in, const uint8_t* scalars, size_t m, size_t n,
                          uint8_t* out32, uint64_t* xyzt_out, uint8_t* status) {
  if (n == 0) return D377_OK;
  const SqrtTables T = d.tables();
  const LongPlan plan = long_plan(m);
  const size_t np = n * plan.g;
  if (!codec_chunked_ok(d))
    return fail(D377_ERR_INIT, "residency of %s does not match the lane sets of the scratch areas", "k_compress_chunked");
  GuardScope vb{d.vb_guard, s};                              // the lane-set areas, the table scratch, the partials: queue behind their last user
  int rc;
  uint64_t* partials = nullptr;
  if ((rc = long_sums_partials(d, s, n, plan.g, &partials))) return rc;

  // ---- phase 1: the chains.  The route by the number of PARTIAL sums, batch_msm.hip's rule: up to four per SIMD a wave each
  if (np <= sums_wave_max(d)) {                              // (launch_plan.hpp)
    if ((rc = vb.acquire())) return rc;
    const size_t lds = plan.b * row::RQ_TAB_ENTRIES * RQ_WORDS * sizeof(uint32_t);
    if (encoded) hipLaunchKernelGGL(k_msm_long_wave<true>, dim3((unsigned)np), dim3(64), lds, s, T, pts_in, scalars, plan, np, partials, status);
    else hipLaunchKernelGGL(k_msm_long_wave<false>, dim3((unsigned)np), dim3(64), lds, s, T, pts_in, scalars, plan, np, partials, status);
    HIP_TRY(hipGetLastError());
  } else {
    const void* fn = encoded ? reinterpret_cast<const void*>(k_msm_long_lane<true>) : reinterpret_cast<const void*>(k_msm_long_lane<false>);
    int& lds = d.bml_lds[encoded ? 1 : 0];
    if ((rc = lane_residency(fn, "k_msm_long_lane", encoded, lds))) return rc;
    // the table scratch of the small sums' lane kernel, for b terms per lane
    uint32_t *tab, *dig;
    if ((rc = straus_scratch_reserve(d, s, plan.b,
           "batch_msm_long: the table scratch must grow, which cannot happen inside a stream capture",
           "batch_msm_long: hipMalloc of the table scratch failed (0.23 GB per term of a group on 256 CUs)", &tab, &dig))) return rc;
    if ((rc = vb.acquire())) return rc;
    int grid;
    const DcbScratch dcb = lane_chunks(d, np, &grid);
    if (encoded)
      hipLaunchKernelGGL(k_msm_long_lane<true>, dim3((unsigned)grid), dim3(BLOCK), lds, s, T, pts_in, scalars, plan, np, partials, status, tab, dig, dcb);
    else
      hipLaunchKernelGGL(k_msm_long_lane<false>, dim3((unsigned)grid), dim3(BLOCK), lds, s, T, pts_in, scalars, plan, np, partials, status, tab, dig, dcb);
    HIP_TRY(hipGetLastError());
  }

  // ---- phases 2 and 3: the fold levels, then the sums' Encodings (msm_long_fold.hpp)
  if ((rc = long_sums_fold_compress(d, s, n, plan.g, out32, xyzt_out))) return rc;
  return vb.finish();
}

// one device's slice of a host batch: copies in, kernels, copies out, synchronised
int batch_msm_long_one(DeviceState& d, bool encoded, const uint8_t* pts_in, const uint8_t* scalars, size_t m, size_t n, uint8_t* out32,
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
    if ((r = batch_msm_long_launch(d, d.stream, encoded, d.buf[0], d.buf[1], m, n, d.buf[2], xyzt_dev, d.buf[3]))) return r;
    if ((r = sums_out_copy(d, n, out32, xyzt_out))) return r;
    if (encoded) HIP_TRY(hipMemcpyAsync(status, d.buf[3], terms, hipMemcpyDeviceToHost, d.stream));
    return D377_OK;
  });
}

// What the host and the resident forms check first, in the documented order and before any device is touched: m, null
// buffers (n > 0), ctx.
int check_args(d377_ctx* ctx, bool encoded, const void* pts_in, const uint8_t* scalars, size_t m, size_t n, const uint8_t* out32,
               const uint8_t* status) {
  if (m < 1 || m > BML_MAX)
    return fail_size(D377_ERR_ARG, "batch_msm_long: m = %zu: 1 .. 4096 terms per sum (D377_BATCH_MSM_LONG_MAX_TERMS); d377_msm for longer sums", m);
  if (n) {
    if (!pts_in) return fail(D377_ERR_ARG, "batch_msm_long: null buffer: %s", encoded ? "enc32" : "xyzt");
    if (!scalars) return fail(D377_ERR_ARG, "batch_msm_long: null buffer: %s", "scalar32");
    if (!out32) return fail(D377_ERR_ARG, "batch_msm_long: null buffer: %s", "enc32_out");
    if (encoded && !status) return fail(D377_ERR_ARG, "batch_msm_long: null buffer: %s", "status");
  }
  if (!ctx) return fail(D377_ERR_ARG, "%s", "batch_msm_long: null context (ctx)");
  return D377_OK;
}

// host pointers
int batch_msm_long_host(d377_ctx* ctx, bool encoded, const void* pts_in, const uint8_t* scalars, size_t m, size_t n, uint8_t* out32,
                        uint64_t* xyzt_out, uint8_t* status) {
  int rc;
  if ((rc = check_args(ctx, encoded, pts_in, scalars, m, n, out32, status))) return rc;
  if (n == 0) return D377_OK;
  if (m <= BML_GROUP_MAX)                                     // one chain per sum: the small sums' call, the same bytes
    return encoded ? d377_batch_msm_small_encoded(ctx, (const uint8_t*)pts_in, scalars, m, n, out32, xyzt_out, status)
                   : d377_batch_msm_small(ctx, (const uint64_t*)pts_in, scalars, m, n, out32, xyzt_out);
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t rec = encoded ? 32 : 128;
  // contiguous slices of the SUMS over the context's devices (host_state.hpp: slice_over_devices)
  return slice_over_devices(ctx, n, [&](size_t k, size_t lo, size_t cnt) {
    return batch_msm_long_one(ctx->devs[k], encoded, (const uint8_t*)pts_in + lo * m * rec, scalars + lo * m * 32, m, cnt, out32 + lo * 32,
                              xyzt_out ? xyzt_out + lo * 16 : nullptr, encoded ? status + lo * m : nullptr);
  });
}

// device pointers and a stream (include/decaf377_amd_long_sums.h): the host form's checks, then dev and the alignment; enqueue
// and return.  m <= 8 is the small sums' `_dev` call, as on the host; longer sums are batch_msm_long_launch under ctx->mu.
int batch_msm_long_resident(d377_ctx* ctx, int dev, void* stream, bool encoded, const void* pts_in, const uint8_t* scalars, size_t m,
                            size_t n, uint8_t* out32, uint64_t* xyzt_out, uint8_t* status) {
  int rc;
  if ((rc = check_args(ctx, encoded, pts_in, scalars, m, n, out32, status))) return rc;
  if (dev < 0 || (size_t)dev >= ctx->devs.size()) return fail(D377_ERR_ARG, "%s", "batch_msm_long: dev is not a device of this context");
  if (!aligned16(pts_in) || !aligned16(scalars) || !aligned16(out32) || !aligned16(xyzt_out))
    return fail(D377_ERR_ARG, "%s", "batch_msm_long: device record buffers must be 16-byte aligned");
  if (n == 0) return D377_OK;
  if (m <= BML_GROUP_MAX)
    return encoded ? d377_batch_msm_small_encoded_dev(ctx, dev, stream, (const uint8_t*)pts_in, scalars, m, n, out32, xyzt_out, status)
                   : d377_batch_msm_small_dev(ctx, dev, stream, (const uint64_t*)pts_in, scalars, m, n, out32, xyzt_out);
  if (n > SIZE_MAX / 128 / m) return fail(D377_ERR_ARG, "%s", "batch_msm_long: n x m overflows");
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceState& d = ctx->devs[(size_t)dev];
  HIP_TRY(hipSetDevice(d.id));
  return batch_msm_long_launch(d, (hipStream_t)stream, encoded, pts_in, scalars, m, n, out32, xyzt_out, status);
}

}  // namespace

extern "C" {

int d377_batch_msm_long(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalar32, size_t m, size_t n, uint8_t* enc32_out,
                        uint64_t* xyzt_out) {
  return batch_msm_long_host(ctx, false, xyzt, scalar32, m, n, enc32_out, xyzt_out, nullptr);
}
int d377_batch_msm_long_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, size_t m, size_t n, uint8_t* enc32_out,
                                uint64_t* xyzt_out, uint8_t* status) {
  return batch_msm_long_host(ctx, true, enc32, scalar32, m, n, enc32_out, xyzt_out, status);
}
int d377_batch_long_msm_resident(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalar32, size_t m, size_t n,
                                 uint8_t* enc32_out, uint64_t* xyzt_out) {
  return batch_msm_long_resident(ctx, dev, stream, false, xyzt, scalar32, m, n, enc32_out, xyzt_out, nullptr);
}
int d377_batch_long_msm_encoded_resident(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalar32, size_t m,
                                         size_t n, uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status) {
  return batch_msm_long_resident(ctx, dev, stream, true, enc32, scalar32, m, n, enc32_out, xyzt_out, status);
}

}  // extern "C"
