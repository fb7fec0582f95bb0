// batch_msm_segmented.hip -- d377_batch_segmented_msm (include/decaf377_amd_segmented_sums.h): many multiscalar sums of ANY
// length each (0 .. 2^20 terms), delimited by offsets, by the Straus chains of batch_msm_long.hip (gfx950).
//
// The bucket pipeline of d377_batch_ragged_msm pays a workgroup per (window, sum) and 2^(window-1) buckets per sum whatever the
// sum's length; here a sum of L terms costs ceil(L / 8) chains.  The cut, the slot spaces and every lookup are
// msm_segmented_plan.hpp's; nothing is built on the host, so the resident forms enqueue kernels that read the offsets on the
// device and nothing else:
//
//   k_seg_lane    one lane per chain SLOT under the lane-set machinery (dcb.hpp), straus.hpp's chain with the lane's own slot
//                 count, the table scratch of batch_msm.hip's lane kernel sized for the call's largest b; a dead slot reads
//                 nothing and writes nothing
//   k_seg_wave    one wave per chain slot (straus_tab.hpp), up to four slots per SIMD
//   k_seg_fold    slot-indexed: one lane adds up to BML_FOLD consecutive records of one sum (ge_add_raw_words), found by the same
//                 search; once per level while some sum has more than BML_FOLD records (the count by value, from the longest sum)
//   k_seg_last    sum-indexed, n lanes: a sum's <= BML_FOLD records into record i of the compact array or of xyzt_out; the
//                 identity record for an empty sum
// and the chunked compressor (codec_chunked.hip) over the n compact records.  The records live in the long sums' partials
// area (msm_long_fold.hpp), under the lane-set guard like everything here.
//
// KNOWN COST, unmeasured: the lanes of a wave of k_seg_lane run 1 .. 8 slots each, so the wave takes as long as its longest
// chain; sums below 8 terms leave table scratch unused.  Chains are neither sorted nor binned by length.
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
#include "msm_long_fold.hpp"
#include "msm_ragged_plan.hpp"
#include "msm_segmented_plan.hpp"

using namespace d377;

namespace {

static_assert(SEG_MAX_TERMS == D377_BATCH_SEGMENTED_MSM_MAX_TERMS && SEG_MAX_TERMS == RSUM_MAX_TERMS, "the limit of the ragged call");
static_assert(BML_GROUP_MAX == D377_BATCH_MSM_MAX_TERMS, "a chain is one chain of the small sums");
static_assert(VB_ENTRIES == 9, "straus_sum stores entries 0 .. 8 of every point's table");

// what every kernel is told about the call, by value, from the HOST offsets
struct SegCall {
  const uint64_t* off;                   // n + 1 offsets on the device; the record buffers begin at term off[0]
  size_t n;
  uint64_t terms;
  int bmax;
};

// ---- one lane per chain slot ------------------------------------------------------------------------------------------------
// slots = floor(terms / 8) + n.  status: one byte per TERM, written for live slots of live chains only.
template <bool ENCODED>
__global__ void __launch_bounds__(BLOCK, WAVES_PER_SIMD)
k_seg_lane(SqrtTables T, const void* pts_in, const uint8_t* scalar32, SegCall call, size_t slots, uint64_t* partials, uint8_t* status,
           uint32_t* tab, uint32_t* dig, DcbScratch dcb) {
  __shared__ uint32_t lds_pow_[ENCODED ? POW_TAB * NL * BLOCK : 1];
  LdsPowTab pt;
  pt.col = lds_pow_ + (ENCODED ? threadIdx.x : 0);
  D377_DCB_BEGIN(partials);                                  // (no compressor here: the chunk walk never writes through io.out32)
  StrausTab st{tab, dig, (size_t)dcb.nslots * BLOCK, io.lane};
  dcb_rounds<0, false>(slots, io, pt,
    [&](size_t, int) {},
    [&](size_t i, int, const uint32_t (*)[8], bool) {
      const SegChain c = seg_chain(call.off, call.n, call.terms, call.bmax, (uint64_t)i);
      if (!c.live) return;                                   // a dead slot: nothing read, nothing written
      const size_t first = (size_t)c.first;
      const int live = c.count;                              // 1 .. b; the slots from `live` on are past the end of the sum
      const ge r = straus_sum(st, c.b, [&](int p, uint32_t k[8]) {
        if (p < live) { load32(scalar32, first + (size_t)p, k); return; }
#pragma unroll
        for (int w = 0; w < 8; ++w) k[w] = 0;                 // a dead slot of the chain: no scalar read
      }, [&](int p, ge* g) -> bool {
        if (p >= live) { *g = ge_identity(); return true; }   // a dead slot of the chain: no point read, no status write
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

// ---- one wave per chain slot ------------------------------------------------------------------------------------------------
using row::RQ_WORDS;
template <bool ENCODED>
__global__ void __launch_bounds__(64)
k_seg_wave(SqrtTables T, const void* pts_in, const uint8_t* scalar32, SegCall call, size_t slots, uint64_t* partials, uint8_t* status) {
  extern __shared__ uint32_t tab[];                                // bmax tables of RQ_TAB_ENTRIES x RQ_WORDS words
  __shared__ uint32_t xrec[2 * RQ_WORDS];
  __shared__ uint32_t sdg[BML_GROUP_MAX][8];
  const size_t slot = blockIdx.x;                                  // grid = slots
  if (slot >= slots) return;
  const SegChain c = seg_chain(call.off, call.n, call.terms, call.bmax, (uint64_t)slot);   // the same in every lane
  if (!c.live) return;                                             // the whole workgroup: no barrier has been met
  const ge r = straus_wave_sum<ENCODED>(T, pts_in, scalar32, (size_t)c.first, c.count, status, tab, xrec, sdg);
  if (threadIdx.x == 0) store_ge_mont256(partials, slot, ge_double_fast(r, true));
}

// adds the records [lo, lo + cnt) of `in`, cnt >= 1, into record `at` of `out`
__device__ __forceinline__ void seg_add_records(const uint64_t* in, size_t lo, int cnt, uint64_t* out, size_t at) {
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
  store_record128(out, at, acc);
}

// ---- a slot-indexed fold level: the S_out slots of level `level` + 1 from the S_in of `level` -----------------------------------
__global__ void __launch_bounds__(BLOCK)
k_seg_fold(SegCall call, int level, const uint64_t* in, size_t S_in, uint64_t* out, size_t S_out) {
  for (size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x; p < S_out; p += (size_t)gridDim.x * BLOCK) {
    const SegFold f = seg_fold(call.off, call.n, level, S_in, (uint64_t)p);
    if (f.live) seg_add_records(in, (size_t)f.lo, f.count, out, p);
  }
}

// ---- the last level: lane i adds the <= BML_FOLD records sum i has at `levels` into record i of `out` ---------------------------
__global__ void __launch_bounds__(BLOCK)
k_seg_last(SegCall call, int levels, const uint64_t* in, size_t S_in, uint64_t* out) {
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < call.n; i += (size_t)gridDim.x * BLOCK) {
    const SegFold f = seg_last(call.off, i, levels, S_in);
    if (f.live) seg_add_records(in, (size_t)f.lo, f.count, out, i);
    else store_ge_mont256(out, i, ge_identity());                  // an empty sum
  }
}

// ------------------------------------------------------------------------------ host side ---
// bytes of table scratch the lane route reserves (batch_host.hpp: straus_scratch_reserve)
size_t seg_table_bytes(const DeviceState& d, int bmax) {
  return (d.resident_lanes() * (size_t)bmax * VB_ENTRIES * BM_ENTRY_WORDS + d.resident_lanes() * BM_WINDOWS) * sizeof(uint32_t);
}

// Everything on device pointers, enqueued on `s`; the caller holds ctx->mu and has selected the device.  off: the n + 1 offsets
// on the host (checked; off[0] need not be 0 here: a device's slice of a host call); off_dev: the same values on the device, or
// null: the launch uploads `off` behind the records of the partials area (the host forms).  The record buffers begin at term
// off[0].
int seg_launch(DeviceState& d, hipStream_t s, bool encoded, const void* pts_in, const uint8_t* scalars, const uint64_t* off,
               const uint64_t* off_dev, size_t n, uint8_t* out32, uint64_t* xyzt_out, uint8_t* status) {
  if (n == 0) return D377_OK;
  const SqrtTables T = d.tables();
  const SegPlan sp = seg_plan(off, n);
  if (!codec_chunked_ok(d))
    return fail(D377_ERR_INIT, "residency of %s does not match the lane sets of the scratch areas", "k_compress_chunked");
  GuardScope vb{d.vb_guard, s};                              // the lane-set areas, the table scratch, the partials: queue behind their last user
  int rc;
  uint64_t* area = nullptr;
  if ((rc = long_sums_partials_records(d, s, sp.records, off_dev ? 0 : (n + 1) * 8, &area))) return rc;
  const bool wave = sp.chain_slots <= sums_wave_max(d);      // (launch_plan.hpp) the route by the number of SLOTS
  uint32_t *tab = nullptr, *dig = nullptr;
  int lds_pad = 0;
  if (sp.terms && !wave) {
    const void* fn = encoded ? reinterpret_cast<const void*>(k_seg_lane<true>) : reinterpret_cast<const void*>(k_seg_lane<false>);
    int& lds = d.seg_lds[encoded ? 1 : 0];
    if ((rc = lane_residency(fn, "k_seg_lane", encoded, lds))) return rc;
    lds_pad = lds;
    if ((rc = straus_scratch_reserve(d, s, (size_t)sp.bmax,
           "batch_segmented_msm: the table scratch must grow, which cannot happen inside a stream capture",
           "batch_segmented_msm: hipMalloc of the table scratch failed (0.23 GB per term of a chain on 256 CUs)", &tab, &dig))) return rc;
  }
  if ((rc = vb.acquire())) return rc;
  if (!off_dev) {
    uint64_t* up = area + sp.records * 16;
    HIP_TRY(hipMemcpyAsync(up, off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    off_dev = up;
  }
  const SegCall call{off_dev, n, sp.terms, sp.bmax};

  // ---- phase 1: the chains, into the slots of level 0
  if (sp.terms && wave) {
    const size_t lds = (size_t)sp.bmax * row::RQ_TAB_ENTRIES * RQ_WORDS * sizeof(uint32_t);
    if (encoded) hipLaunchKernelGGL(k_seg_wave<true>, dim3((unsigned)sp.chain_slots), dim3(64), lds, s, T, pts_in, scalars, call, sp.chain_slots, area, status);
    else hipLaunchKernelGGL(k_seg_wave<false>, dim3((unsigned)sp.chain_slots), dim3(64), lds, s, T, pts_in, scalars, call, sp.chain_slots, area, status);
    HIP_TRY(hipGetLastError());
  } else if (sp.terms) {
    int grid;
    const DcbScratch dcb = lane_chunks(d, sp.chain_slots, &grid);
    if (encoded)
      hipLaunchKernelGGL(k_seg_lane<true>, dim3((unsigned)grid), dim3(BLOCK), lds_pad, s, T, pts_in, scalars, call, sp.chain_slots, area, status, tab, dig, dcb);
    else
      hipLaunchKernelGGL(k_seg_lane<false>, dim3((unsigned)grid), dim3(BLOCK), lds_pad, s, T, pts_in, scalars, call, sp.chain_slots, area, status, tab, dig, dcb);
    HIP_TRY(hipGetLastError());
  }

  // ---- phase 2: the slot-indexed levels, then the last level into the compact records (or the caller's)
  for (int l = 0; l < sp.levels; ++l) {
    hipLaunchKernelGGL(k_seg_fold, dim3((unsigned)fold_grid(d, sp.space[l + 1])), dim3(BLOCK), 0, s, call, l, area + sp.base[l] * 16, sp.space[l],
                       area + sp.base[l + 1] * 16, sp.space[l + 1]);
    HIP_TRY(hipGetLastError());
  }
  uint64_t* sums = xyzt_out ? xyzt_out : area + sp.base[sp.levels + 1] * 16;
  hipLaunchKernelGGL(k_seg_last, dim3((unsigned)fold_grid(d, n)), dim3(BLOCK), 0, s, call, sp.levels, area + sp.base[sp.levels] * 16, sp.space[sp.levels], sums);
  HIP_TRY(hipGetLastError());

  // ---- phase 3: the sums' Encodings, in chunks with batched inversions (codec_chunked.hip)
  int grid;
  const DcbScratch dcb = lane_chunks(d, n, &grid);
  if ((rc = codec_chunked_launch(d, s, false, sums, n, out32, nullptr, grid, dcb))) return rc;
  return vb.finish();
}

// What every form checks first, in the documented order and before any device is touched: n, null offsets, the offsets'
// values, null buffers, ctx.  plan_only: d377_segmented_msm_plan, which has no buffers.
int seg_check_args(d377_ctx* ctx, bool encoded, bool plan_only, const void* pts_in, const uint8_t* scalars, const uint64_t* off, size_t n,
                   const uint8_t* out32, const uint8_t* status) {
  if (n > (SIZE_MAX / 128) - 1) {
    snprintf(d377_g_err, sizeof d377_g_err, "batch_segmented_msm: n = %zu: n + 1 offsets and n records overflow", n);
    return D377_ERR_ARG;
  }
  if (n) {
    if (!off) return fail(D377_ERR_ARG, "batch_segmented_msm: null buffer: %s", "offsets");
    if (off[0] != 0) {
      snprintf(d377_g_err, sizeof d377_g_err, "batch_segmented_msm: offsets [0] = %llu (sum 0): the first of the offsets must be 0",
               (unsigned long long)off[0]);
      return D377_ERR_ARG;
    }
    const size_t bad = rsum_first_bad_sum(off, n);
    if (bad < n) {
      if (off[bad + 1] < off[bad])
        snprintf(d377_g_err, sizeof d377_g_err, "batch_segmented_msm: offsets decrease at sum %zu: %llu after %llu", bad,
                 (unsigned long long)off[bad + 1], (unsigned long long)off[bad]);
      else
        snprintf(d377_g_err, sizeof d377_g_err,
                 "batch_segmented_msm: offsets give sum %zu %llu terms: at most 1048576 per sum (D377_BATCH_SEGMENTED_MSM_MAX_TERMS); d377_msm "
                 "for one longer sum", bad, (unsigned long long)(off[bad + 1] - off[bad]));
      return D377_ERR_ARG;
    }
    if (off[n] > SIZE_MAX / 128) return fail(D377_ERR_ARG, "%s", "batch_segmented_msm: offsets [n] x 128 overflows");
    if (!plan_only) {
      if (off[n]) {
        if (!pts_in) return fail(D377_ERR_ARG, "batch_segmented_msm: null buffer: %s", encoded ? "enc32" : "xyzt");
        if (!scalars) return fail(D377_ERR_ARG, "batch_segmented_msm: null buffer: %s", "scalar32");
      }
      if (!out32) return fail(D377_ERR_ARG, "batch_segmented_msm: null buffer: %s", "enc32_out");
      if (off[n] && encoded && !status) return fail(D377_ERR_ARG, "batch_segmented_msm: null buffer: %s", "status");
    }
  }
  if (!ctx) return fail(D377_ERR_ARG, "%s", "batch_segmented_msm: null context (ctx)");
  return D377_OK;
}

// one device's slice of a host batch: sums lo .. lo + n - 1 (off = offsets + lo); copies in, the kernels, copies out, synchronised
int seg_one(DeviceState& d, bool encoded, const uint8_t* pts_in, const uint8_t* scalars, const uint64_t* off, size_t n, uint8_t* out32,
            uint64_t* xyzt_out, uint8_t* status) {
  if (n == 0) return D377_OK;
  return device_slice(d, [&]() -> int {
    const size_t rec = encoded ? 32 : 128, terms = (size_t)(off[n] - off[0]);
    int r;
    uint64_t* xyzt_dev;
    if ((r = ensure(d, 0, terms * rec))) return r;
    if ((r = ensure(d, 1, terms * 32))) return r;
    if ((r = sums_out_reserve(d, n, xyzt_out != nullptr, &xyzt_dev))) return r;
    if (encoded && (r = ensure(d, 3, terms))) return r;
    if (terms) {
      HIP_TRY(hipMemcpyAsync(d.buf[0], pts_in, terms * rec, hipMemcpyHostToDevice, d.stream));
      HIP_TRY(hipMemcpyAsync(d.buf[1], scalars, terms * 32, hipMemcpyHostToDevice, d.stream));
    }
    if ((r = seg_launch(d, d.stream, encoded, d.buf[0], d.buf[1], off, nullptr, n, d.buf[2], xyzt_dev, encoded ? d.buf[3] : nullptr))) return r;
    if ((r = sums_out_copy(d, n, out32, xyzt_out))) return r;
    if (encoded && terms) HIP_TRY(hipMemcpyAsync(status, d.buf[3], terms, hipMemcpyDeviceToHost, d.stream));
    return D377_OK;
  });
}

int seg_host(d377_ctx* ctx, bool encoded, const void* pts_in, const uint8_t* scalars, const uint64_t* off, size_t n, uint8_t* out32,
             uint64_t* xyzt_out, uint8_t* status) {
  int rc;
  if ((rc = seg_check_args(ctx, encoded, false, pts_in, scalars, off, n, out32, status))) return rc;
  if (n == 0) return D377_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t rec = encoded ? 32 : 128, nd = ctx->devs.size();
  // contiguous slices of the SUMS, cut where the TERMS are shared out evenly (msm_ragged_plan.hpp: rsum_device_cut): one unit per device
  return slice_over_devices(ctx, nd, [&](size_t k, size_t, size_t) {
    const size_t lo = rsum_device_cut(off, n, nd, k), hi = rsum_device_cut(off, n, nd, k + 1);
    const size_t t0 = (size_t)off[lo];
    return seg_one(ctx->devs[k], encoded, (const uint8_t*)pts_in + t0 * rec, scalars + t0 * 32, off + lo, hi - lo, out32 + lo * 32,
                   xyzt_out ? xyzt_out + lo * 16 : nullptr, encoded ? status + t0 : nullptr);
  });
}

int seg_resident(d377_ctx* ctx, int dev, void* stream, bool encoded, const void* pts_in, const uint8_t* scalars, const uint64_t* off,
                 const uint64_t* off_dev, size_t n, uint8_t* out32, uint64_t* xyzt_out, uint8_t* status) {
  int rc;
  if ((rc = seg_check_args(ctx, encoded, false, pts_in, scalars, off, n, out32, status))) return rc;
  if (dev < 0 || (size_t)dev >= ctx->devs.size()) return fail(D377_ERR_ARG, "%s", "batch_segmented_msm: dev is not a device of this context");
  if (n && !off_dev) return fail(D377_ERR_ARG, "batch_segmented_msm: null buffer: %s", "offsets_dev");
  if ((reinterpret_cast<uintptr_t>(off_dev) & 7u) != 0) return fail(D377_ERR_ARG, "%s", "batch_segmented_msm: offsets_dev must be 8-byte aligned");
  if (!aligned16(pts_in) || !aligned16(scalars) || !aligned16(out32) || !aligned16(xyzt_out))
    return fail(D377_ERR_ARG, "%s", "batch_segmented_msm: device record buffers must be 16-byte aligned");
  if (n == 0) return D377_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceState& d = ctx->devs[(size_t)dev];
  HIP_TRY(hipSetDevice(d.id));
  return seg_launch(d, (hipStream_t)stream, encoded, pts_in, scalars, off, off_dev, n, out32, xyzt_out, status);
}

}  // namespace

extern "C" {

int d377_batch_segmented_msm(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalar32, const uint64_t* offsets, size_t n,
                             uint8_t* enc32_out, uint64_t* xyzt_out) {
  return seg_host(ctx, false, xyzt, scalar32, offsets, n, enc32_out, xyzt_out, nullptr);
}
int d377_batch_segmented_msm_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, const uint64_t* offsets, size_t n,
                                     uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status) {
  return seg_host(ctx, true, enc32, scalar32, offsets, n, enc32_out, xyzt_out, status);
}
int d377_batch_segmented_msm_resident(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalar32,
                                      const uint64_t* offsets, const uint64_t* offsets_dev, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out) {
  return seg_resident(ctx, dev, stream, false, xyzt, scalar32, offsets, offsets_dev, n, enc32_out, xyzt_out, nullptr);
}
int d377_batch_segmented_msm_encoded_resident(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalar32,
                                              const uint64_t* offsets, const uint64_t* offsets_dev, size_t n, uint8_t* enc32_out,
                                              uint64_t* xyzt_out, uint8_t* status) {
  return seg_resident(ctx, dev, stream, true, enc32, scalar32, offsets, offsets_dev, n, enc32_out, xyzt_out, status);
}
int d377_segmented_msm_plan(d377_ctx* ctx, int dev, const uint64_t* offsets, size_t n, uint64_t* chain_slots, uint64_t* chains,
                            int* fold_levels, int* max_slots_per_chain, uint64_t* scratch_bytes, int* advised_route) {
  int rc;
  if ((rc = seg_check_args(ctx, false, true, nullptr, nullptr, offsets, n, nullptr, nullptr))) return rc;
  if (dev < 0 || (size_t)dev >= ctx->devs.size()) return fail(D377_ERR_ARG, "%s", "batch_segmented_msm: dev is not a device of this context");
  std::lock_guard<std::mutex> lock(ctx->mu);
  const DeviceState& d = ctx->devs[(size_t)dev];
  const SegPlan sp = seg_plan(offsets, n);
  if (chain_slots) *chain_slots = sp.chain_slots;
  if (chains) *chains = sp.chains;
  if (fold_levels) *fold_levels = sp.levels;
  if (max_slots_per_chain) *max_slots_per_chain = sp.bmax;
  if (scratch_bytes)
    *scratch_bytes = (uint64_t)sp.records * 128 + ((sp.terms && sp.chain_slots > sums_wave_max(d)) ? seg_table_bytes(d, sp.bmax) : 0);
  if (advised_route) *advised_route = sp.advised_route;
  return D377_OK;
}

}  // extern "C"
