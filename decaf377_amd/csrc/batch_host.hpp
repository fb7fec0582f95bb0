// batch_host.hpp -- the host launch path the batched-sum units share (batch_msm.hip, batch_msm_long.hip,
// batch_msm_long_indexed.hip, batch_msm_mixed.hip, fixed_bases.hip): the residency check of a lane kernel, the Straus table scratch, the DcbScratch of a lane-set kernel's chunk deal (launch_plan.hpp) and
// the frame of one device's slice of a host-pointer call.  (The fan-out over the devices is host_state.hpp's
// slice_over_devices.)  Everything here runs under ctx->mu.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "dcb.hpp"
#include "straus.hpp"
#include "host_state.hpp"

namespace d377 {

// Residency of a lane kernel against the lane sets (as d377_ctx_create checks the kernels of d377.hip): at most
// WAVES_PER_SIMD workgroups per CU, padded with dynamic LDS where registers alone would let more in.  Once per device and
// instantiation: `lds` is that kernel's cache in DeviceState (-1 = not asked yet) and receives the padding.
inline int lane_residency(const void* fn, const char* name, int bits, int& lds) {
  if (lds >= 0) return D377_OK;
  int nb = 0;
  HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, BLOCK, 0));
  int pad = 0;
  if (nb > WAVES_PER_SIMD) {
    pad = (160 * 1024) / (WAVES_PER_SIMD + 1) + 1024;
    if (pad > 64 * 1024) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, pad));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, BLOCK, (size_t)pad));
  }
  if (getenv("D377_DEBUG_RESIDENCY"))
    fprintf(stderr, "d377: %s<%d>: %d workgroups per CU with %d bytes of LDS padding\n", name, bits, nb, pad);
  if (nb < 1 || nb > WAVES_PER_SIMD)
    return fail(D377_ERR_INIT, "residency of %s does not match the lane sets of the scratch areas", name);
  lds = pad;
  return D377_OK;
}

// The Straus table scratch d.bm_scratch for `terms` tables per resident lane (straus_tab.hpp: the tables, then the digit
// words), grown if it is smaller: *tab and *dig are the two parts.  The area may not grow inside a stream capture
// (D377_ERR_ARG, text `in_capture`); a failed allocation is D377_ERR_HIP with text `no_memory`.  Launches on `s`; the caller
// holds the scope of the lane-set guard (GuardScope on d.vb_guard), not yet acquired.
inline int straus_scratch_reserve(DeviceState& d, hipStream_t s, size_t terms, const char* in_capture, const char* no_memory,
                                  uint32_t** tab, uint32_t** dig) {
  const size_t tab_words = d.resident_lanes() * terms * VB_ENTRIES * BM_ENTRY_WORDS;
  const size_t need = (tab_words + d.resident_lanes() * BM_WINDOWS) * sizeof(uint32_t);
  int rc;
  if ((rc = d.bm_scratch.reserve(d.vb_guard, s, need, SLACK_TABLE_SCRATCH, in_capture, no_memory))) return rc;
  *tab = d.bm_scratch.as<uint32_t>();
  *dig = *tab + tab_words;
  return D377_OK;
}

// launch_plan.hpp restates these (it is compiled without the device headers)
static_assert(PLAN_BLOCK == BLOCK && PLAN_WAVES_PER_SIMD == WAVES_PER_SIMD && PLAN_DCB_K == DCB_K && PLAN_DCB_KMAX == DCB_KMAX &&
              PLAN_DCB_K_LONG == DCB_K_LONG && PLAN_FB_SETS == FB_SETS && PLAN_FB_K == FB_K && PLAN_FB_WIDE_GENERATIONS == FB_WIDE_GENERATIONS,
              "launch_plan.hpp");

// The DcbScratch of a lane-set launch: the device's areas around the numbers of the plan's chunk deal (launch_plan.hpp).
inline DcbScratch lane_scratch(const DeviceState& d, const LaneDeal& c) {
  DcbScratch dcb{d.dcb_scratch, d.slot_pool, c.nslots, c.per_lane, d.dcb_sets * BLOCK, c.extra, d.pool_health};
  dcb.prio = c.prio;
  return dcb;
}
// The chunks of a lane-set kernel of the sums over `count` elements, at most kmax rounds per chunk: the launch's grid and its
// DcbScratch (lane_deal, the form that reads no tuning key).
inline DcbScratch lane_chunks(const DeviceState& d, size_t count, int* grid, int kmax = DCB_K) {
  const LaneDeal c = lane_deal(d, count, WAVES_PER_SIMD, kmax, false);
  *grid = c.grid;
  return lane_scratch(d, c);
}

// One device's slice of a host-pointer call: body() stages the inputs, launches on d.stream and enqueues the copies out; the
// frame selects the device, brackets the body with the starvation check, synchronises and gives the verdict.  On an error
// nothing is left in flight (SyncOnError).
template <class Body>
int device_slice(DeviceState& d, Body&& body) {
  HIP_TRY(hipSetDevice(d.id));
  int rc = D377_OK;
  SyncOnError guard{&rc, d.id, d.stream, nullptr};
  rc = [&]() -> int {
    StarveCheck starve{d, d.stream};
    int r;
    if ((r = starve.before())) return r;
    if ((r = body())) return r;
    if ((r = starve.after())) return r;
    HIP_TRY(hipStreamSynchronize(d.stream));
    return starve.verdict();
  }();
  return rc;
}

// The staging of a slice's outputs in buf[2]: n Encodings, then n Element records if the caller wants them (*xyzt_dev, else null).
inline int sums_out_reserve(DeviceState& d, size_t n, bool want_xyzt, uint64_t** xyzt_dev) {
  int rc;
  if ((rc = ensure(d, 2, n * (want_xyzt ? 32 + 128 : 32)))) return rc;
  *xyzt_dev = want_xyzt ? reinterpret_cast<uint64_t*>(d.buf[2] + n * 32) : nullptr;
  return D377_OK;
}
// ... and their copies to the caller, enqueued on d.stream
inline int sums_out_copy(DeviceState& d, size_t n, uint8_t* out32, uint64_t* xyzt_out) {
  HIP_TRY(hipMemcpyAsync(out32, d.buf[2], n * 32, hipMemcpyDeviceToHost, d.stream));
  if (xyzt_out) HIP_TRY(hipMemcpyAsync(xyzt_out, d.buf[2] + n * 32, n * 128, hipMemcpyDeviceToHost, d.stream));
  return D377_OK;
}

// ---- the resident (device-pointer) forms of the sums over registered bases (fixed_bases.hip, batch_msm_mixed.hip)
inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// What those forms share once the call's own range and null checks have passed: ctx, dev, the handle,
// the alignment of the record buffers (16 bytes), of the indices (4) and of the verdict (8), then the device is selected.
// The caller holds ctx->mu.
struct ResidentCall {
  DeviceState* d = nullptr;
  const FixedBases* fb = nullptr;
  const uint32_t* tab = nullptr;
};
inline int resident_enter(const char* who, d377_ctx* ctx, int dev, int64_t handle, const void* const* rec16, int nrec, const int* index,
                          const uint64_t* verdict, ResidentCall* rc) {
  if (dev < 0 || (size_t)dev >= ctx->devs.size()) return fail(D377_ERR_ARG, "%s: dev is not a device of this context", who);
  rc->fb = fixed_bases_find(ctx, handle);
  if (!rc->fb) return fail(D377_ERR_ARG, "%s: handle is not a live registration of this context", who);
  for (int k = 0; k < nrec; ++k)
    if (!aligned16(rec16[k])) return fail(D377_ERR_ARG, "%s: device record buffers must be 16-byte aligned", who);
  if (!aligned_to(index, 4)) return fail(D377_ERR_ARG, "%s: base_index must be 4-byte aligned", who);
  if (!aligned_to(verdict, 8)) return fail(D377_ERR_ARG, "%s: verdict must be 8-byte aligned", who);
  rc->d = &ctx->devs[(size_t)dev];
  rc->tab = rc->fb->tab[(size_t)dev];
  HIP_TRY(hipSetDevice(rc->d->id));
  return D377_OK;
}

}  // namespace d377
