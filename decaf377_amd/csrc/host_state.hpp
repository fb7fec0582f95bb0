// host_state.hpp -- per-context / per-device host state shared by the translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/decaf377_amd.h"
#include "curve.hpp"
#include "device_util.hpp"
#include "launch_plan.hpp"
#include "scratch_area.hpp"

namespace d377 {

// The kernels that work in chunks and claim a lane set of the per-device scratch areas (d377.hip: dcb_claim).  At most
// chunk_sets[k] workgroups of kernel k may be resident per CU -- that is how many lane sets it may claim; d377_ctx_create checks
// each with hipOccupancyMaxActiveBlocksPerMultiprocessor and pads the launch's LDS allocation for a kernel whose
// registers and own LDS would let more in (chunk_lds, bytes of dynamic LDS per launch).
enum ChunkKernel { CK_SQRT, CK_ENCODE, CK_HASH, CK_MUL_VAR, CK_MUL_BASE, CK_MUL_VAR_EL, CK_MAP_EL, CK_ENCODE_WIDE, CK_DECOMPRESS, CK_COUNT };

struct DeviceState : PlanDev {               // (launch_plan.hpp: the CU count and the context's overrides, as the launch rules read them)
  int id = -1;
  int chunk_lds[CK_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
  int chunk_blocks[CK_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};     // resident workgroups per CU with that padding (occupancy query)
  int chunk_sets[CK_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};       // lane sets per CU the kernel may claim = the residency it is launched for
  int chunk_k[CK_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};          // elements per lane per shared inversion
  int fb_narrow_lds = 0;                 // LDS padding of the fixed-base kernel's narrow launch (WAVES_PER_SIMD workgroups per CU)
  int msm_enc_chunked = -1;              // msm.hip: may the chunked decoding pass run (its residency matches the lane sets)?  -1 = not asked yet
  int codec_chunked = -1;                // codec_chunked.hip: may its kernels claim lane sets (their residency matches them)?  -1 = not asked yet
  int msm_span_blocks = -1;              // msm.hip: workgroups of k_msm_spans a CU holds (occupancy query), -1 = not asked yet
  int dcb_sets = 0;                      // lane sets of the round-record area and its pool (the largest chunk_sets x CUs)
  int bm_lds[2] = {-1, -1};              // batch_msm.hip: LDS padding of its lane kernel (Element / Encoding form), -1 = not asked yet
  int bml_lds[2] = {-1, -1};             // batch_msm_long.hip: LDS padding of its lane kernel (Element / Encoding form), -1 = not asked yet
  int seg_lds[2] = {-1, -1};             // batch_msm_segmented.hip: the same for its lane kernel
  int bmli_lds = -1;                     // batch_msm_long_indexed.hip: LDS padding of its lane kernel, -1 = not asked yet
  uint8_t* bmli_pool = nullptr;          // batch_msm_long_indexed.hip: the pool's staging area of the host form; grown on demand
  size_t bmli_pool_cap = 0;
  int fx_lds[4] = {-1, -1, -1, -1};      // fixed_bases.hip: LDS padding of its lane kernel per comb width (8 / 12 / 16 / 18), -1 = not asked yet
  int fxi_lds[4] = {-1, -1, -1, -1};     // the same for the lane kernel of the indexed sums
  int bmx_lds[2][4] = {{-1, -1, -1, -1}, {-1, -1, -1, -1}};   // batch_msm_mixed.hip: LDS padding of its lane kernel, [Element / Encoding form][comb width], -1 = not asked yet
  uint32_t* gtab = nullptr;
  uint8_t* s_lookup = nullptr;
  uint32_t* fbase = nullptr;             // the fixed-base comb: null until built (d377.hip ensure_comb: at context creation, or by the first fixed-base call of a lazy context)
  uint32_t* fb_bases = nullptr;          // 2^(fb_bits i) B, the comb builder's window bases
  int fb_bits = FB_BITS;                 // the comb's width: the build's default, or d377_ctx_opts::comb_bits (18 / 21 / 23)
  bool fb_lazy = false;                  // d377_ctx_opts::comb_lazy
  uint32_t* vb_scratch = nullptr;
  uint32_t* vb_identity = nullptr;        // the window tables' shared entry 0 (d377.hip GlobalTab)
  uint8_t* dcb_scratch = nullptr;        // round records of the batched inversions (curve.hpp: dcb_invert_slot, dcb_finish)
  int* slot_pool = nullptr;              // which of the lane sets of the scratch areas are claimed, and by which ticket (dcb.hpp, DcbScratch)
  uint32_t* pool_health = nullptr;       // ticket counter, workgroups that waited long for a set, workgroups that gave up (dcb.hpp)
  int* pool_host = nullptr;              // pinned: where d377_ctx_health / reset_scratch read the pool and the health words
  uint32_t* starve_host = nullptr;       // pinned: the gave-up counter before / after a host-pointer call's kernels (StarveCheck)
  int vb_blocks = 0;
  uint32_t* inv_fail = nullptr;          // device counter of the -DD377_CHECK_INVARIANTS build (always allocated)
  ScratchGuard vb_guard;                 // the lane-set areas and the two areas below
  ScratchArea bm_scratch;                // batch_msm.hip: tables and digit words of the batched small sums, per resident lane; grown on first use
  ScratchArea bml_partials;              // batch_msm_long.hip: the chains' partial sums and the fold levels' records; grown on demand, never shrunk
  hipStream_t stream = nullptr;          // compute stream of the host-pointer entry points
  hipStream_t copy_stream = nullptr;     // PCIe copies of the pipelined host path
  hipStream_t ctl_stream = nullptr;      // highest priority: d377_ctx_health / d377_ctx_reset_scratch (a hardware queue no kernel of ours waits in)
  hipEvent_t ev_in[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
  // grow-only staging buffers for the host-pointer entry points (set 1 = second half of the
  // double buffer used when a large batch is pipelined chunk by chunk)
  uint8_t* buf[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t cap[4] = {0, 0, 0, 0};
  uint8_t* buf2[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t cap2[4] = {0, 0, 0, 0};
  // staging of the sharded device-pointer path (slices of a batch that lives on another device)
  uint8_t* shard[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t shard_cap[4] = {0, 0, 0, 0};
  hipEvent_t ev_shard = nullptr;
  ScratchGuard msm_guard;
  ScratchArea msm_ws;                    // msm.hip: the workspace of the multi-scalar multiplication, one per device
  ScratchArea rsum_offsets;              // msm_ragged.inc: the offsets a host form of the ragged sums uploads (under msm_guard); grown on demand
  SqrtTables tables() const { return SqrtTables{gtab, s_lookup, inv_fail}; }
};

inline int grow(uint8_t*& p, size_t& cap, size_t bytes, size_t slack) {
  if (bytes <= cap) return D377_OK;
  if (p) HIP_TRY(hipFree(p));
  p = nullptr; cap = 0;
  HIP_TRY(hipMalloc(&p, bytes + slack));
  cap = bytes + slack;
  return D377_OK;
}
inline int ensure(DeviceState& d, int slot, size_t bytes) { return grow(d.buf[slot], d.cap[slot], bytes, bytes / 4 + 4096); }
inline int ensure2(DeviceState& d, int slot, size_t bytes) { return grow(d.buf2[slot], d.cap2[slot], bytes, 4096); }
inline int ensure_shard(DeviceState& d, int slot, size_t bytes) { return grow(d.shard[slot], d.shard_cap[slot], bytes, bytes / 4 + 4096); }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Synchronises a set of streams when the enclosing function returns with an error after work has been
// enqueued: no copy into caller memory (or into a local vector) may still be in flight once we return.
struct SyncOnError {
  int* rc;
  int device;
  hipStream_t a, b;
  ~SyncOnError() {
    if (*rc == D377_OK) return;
    char saved[sizeof d377_g_err];
    memcpy(saved, d377_g_err, sizeof saved);            // keep the first error text
    (void)hipSetDevice(device);
    if (a) (void)hipStreamSynchronize(a);
    if (b) (void)hipStreamSynchronize(b);
    memcpy(d377_g_err, saved, sizeof saved);
  }
};

// A host-pointer call must not return D377_OK with records a starved workgroup never wrote (dcb.hpp: after
// DCB_GIVE_UP_TICKS without a lane set a workgroup counts itself in health[2] and leaves).  The call copies the counter
// to pinned memory on its stream before its first kernel and after its last; the call's own final synchronisation
// covers both copies, and verdict() turns a counter that moved into D377_ERR_STARVED.  (A `_dev` launch of another
// stream that starves during the call fails it too: the device's scratch pool is unhealthy either way.)
struct StarveCheck {
  DeviceState& d;
  hipStream_t s;
  int before() { HIP_TRY(hipMemcpyAsync(&d.starve_host[0], d.pool_health + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s)); return D377_OK; }
  int after() { HIP_TRY(hipMemcpyAsync(&d.starve_host[1], d.pool_health + 2, sizeof(uint32_t), hipMemcpyDeviceToHost, s)); return D377_OK; }
  int verdict() const {                                     // after the stream has been synchronised
    if (d.starve_host[1] == d.starve_host[0]) return D377_OK;
    snprintf(d377_g_err, sizeof d377_g_err,
             "%u workgroup(s) found no free lane set for 10 s and left their output records unwritten (device %d): "
             "d377_ctx_health / d377_ctx_reset_scratch", d.starve_host[1] - d.starve_host[0], d.id);
    return D377_ERR_STARVED;
  }
};

// D377_DEBUG_DEVICE_DELAY_MS (tests only): every per-device worker of a multi-device host call sleeps this
// long before it touches its device, which makes "the devices work concurrently" observable on a box
// with a single GPU listed twice.
int debug_device_delay_ms();

// fixed_bases.hip: frees the tables of every registration of d377_fixed_bases_create still alive on the context (d377_ctx_destroy).
// Caller holds no lock; the context is being destroyed, so no other call may be running on it.
struct FixedBases;
void fixed_bases_release_all(d377_ctx* ctx);
// fixed_bases.hip: the live registration `handle` of the context, or null (batch_msm_mixed.hip).  Caller holds ctx->mu.
FixedBases* fixed_bases_find(d377_ctx* ctx, int64_t handle);
// fixed_bases.hip: the verdict on `count` base indices against m bases (index_verdict.hpp), enqueued on `s`: the record's
// initialisation and k_index_verdict.  count == 0 leaves the record (0, none).  Caller holds ctx->mu.
int index_verdict_launch(DeviceState& d, hipStream_t s, const int* base_index, size_t count, int m, uint64_t* verdict);

}  // namespace d377

struct d377_ctx {
  std::vector<d377::DeviceState> devs;
  std::mutex mu;
  d377::Tuning tune;
  std::vector<int> peer;                  // [a][b]: 1 = the same physical device, 2 = peer access a -> b enabled by d377_ctx_create, 0 = none
  std::vector<d377::FixedBases*> fixed;   // the live registrations of d377_fixed_bases_create (under mu): released with the context
  int64_t next_fixed = 1;                 // the next handle d377_fixed_bases_create hands out
};

// One registration of d377_fixed_bases_create: one comb per base on every device of the context, the m combs of a device
// in one allocation (fixed_comb.hpp).  Owned by the context's `fixed` list until d377_fixed_bases_destroy.
namespace d377 {
struct FixedBases {
  int64_t handle = 0;
  size_t m = 0;
  int bits = 0;
  uint64_t bytes = 0;                     // table bytes per device
  std::vector<uint32_t*> tab;             // per device of the context, in its order
};
}  // namespace d377

namespace d377 {
// A host-pointer call's n elements in contiguous slices over the context's devices: f(k, lo, cnt) drives elements
// [lo, lo + cnt) on device k and returns the slice's code.  One device: on the caller's thread.  Several: ceil(n / devices)
// elements per device, each slice driven by its own host thread -- copies from pageable caller memory block the issuing
// thread, so a single thread would run the devices one after another -- and every device has drained before this returns,
// error or not.  -> the first failing device's code, with that worker's thread-local text.  The caller holds ctx->mu.
template <class F>
int slice_over_devices(d377_ctx* ctx, size_t n, F&& f) {
  const size_t nd = ctx->devs.size();
  if (nd == 1) return f((size_t)0, (size_t)0, n);
  const size_t per = (n + nd - 1) / nd;
  std::vector<int> rcs(nd, D377_OK);
  std::vector<std::string> errs(nd);
  std::vector<std::thread> workers;
  const int delay = debug_device_delay_ms();
  for (size_t k = 0; k < nd; ++k) {
    const size_t lo = per * k;
    if (lo >= n) break;
    const size_t cnt = (lo + per <= n) ? per : n - lo;
    workers.emplace_back([&, k, lo, cnt]() {
      if (delay > 0) std::this_thread::sleep_for(std::chrono::milliseconds(delay));
      rcs[k] = f(k, lo, cnt);
      if (rcs[k] != D377_OK) errs[k] = d377_g_err;
    });
  }
  for (auto& w : workers) w.join();
  for (size_t k = 0; k < nd; ++k)
    if (rcs[k] != D377_OK) return fail(rcs[k], "%s", errs[k].c_str());
  return D377_OK;
}
}  // namespace d377
