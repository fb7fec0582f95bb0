// batch_msm_long_indexed.hip -- many multiscalar sums of 1 .. 4096 terms whose terms NAME their points (gfx950):
// out[i] = sum_{j < m} scalar[i m + j] * pool[point_index[i m + j]].
//
// d377_batch_msm_long carries a 128-byte record per term; sums that draw on a common set of points -- a thousand vector
// commitments over the same ad-hoc generators, equations that reuse keys, subsets of one commitment list -- would materialise
// n x m records for it.  Here a term is 36 bytes, an index into a pool of Element records and a scalar, and an index of -1 is
// an absent term, which gives sums of unequal length.  The cut (batch_msm_long_plan.hpp), the table scratch, the partials
// area, the fold and the compressor (msm_long_fold.hpp) are batch_msm_long.hip's; the two chains are that unit's with the
// point gathered through the index, and what a slot is -- live, past the end, absent -- is batch_msm_long_indexed_plan.hpp:
//
//   k_msm_long_indexed_lane   one lane per PARTIAL sum over straus_sum; every chain of a launch runs b slots
//   k_msm_long_indexed_wave   one wave per partial sum in the lane-spread form (row_ops.hpp), tables in LDS: calls of up to
//                             four partial sums per SIMD.  The chain is straus_tab.hpp's straus_wave_sum for Elements with
//                             the gather and the absent terms, written beside it: that function's three units are measured
//                             artefacts and keep their code.
//
// m <= 8 runs on the same kernels with g = 1: then no fold level follows, so the chains also write the caller's Element
// records.  A translation unit of its own, like batch_msm_long.hip.
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
#include "batch_msm_long_indexed_plan.hpp"
#include "msm_long_fold.hpp"

using namespace d377;

namespace {

constexpr size_t BMLI_MAX = D377_BATCH_MSM_LONG_MAX_TERMS;
constexpr size_t BMLI_POOL_MAX = 0x7fffffffu;
static_assert(BML_GROUP_MAX == D377_BATCH_MSM_MAX_TERMS, "a group is one chain of the small sums");
static_assert(VB_ENTRIES == 9, "straus_sum stores entries 0 .. 8 of every point's table");

// ---- one lane per partial sum -----------------------------------------------------------------------------------------------
// np = n g partial sums; partial i = s g + q.  xyzt_out: not null only where g == 1 -- the partial sums are the sums.
__global__ void __launch_bounds__(BLOCK, WAVES_PER_SIMD)
k_msm_long_indexed_lane(SqrtTables T, const uint64_t* pool, uint32_t pool_count, const int* point_index, const uint8_t* scalar32,
                        LongPlan plan, size_t np, uint64_t* partials, uint64_t* xyzt_out, uint32_t* tab, uint32_t* dig, DcbScratch dcb) {
  __shared__ uint32_t lds_pow_[1];
  LdsPowTab pt;
  pt.col = lds_pow_;
  D377_DCB_BEGIN(partials);                                  // (no compressor here: the chunk walk never writes through io.out32)
  StrausTab st{tab, dig, (size_t)dcb.nslots * BLOCK, io.lane};
  dcb_rounds<0, false>(np, io, pt,
    [&](size_t, int) {},
    [&](size_t i, int, const uint32_t (*)[8], bool) {
      const size_t s = i / plan.g, q = i % plan.g;
      const ge r = straus_sum(st, (int)plan.b, [&](int p, uint32_t k[8]) {
        const LongSlot sl = long_indexed_slot(plan, s, q, p, point_index, pool_count);
        if (sl.kind == SLOT_LIVE) { load32(scalar32, sl.term, k); return; }
#pragma unroll
        for (int w = 0; w < 8; ++w) k[w] = 0;                 // a dead slot: no scalar read
      }, [&](int p, ge* g) -> bool {
        const LongSlot sl = long_indexed_slot(plan, s, q, p, point_index, pool_count);
        if (sl.kind != SLOT_LIVE) { *g = ge_identity(); return true; }   // a dead slot: no point read
        *g = load_ge_mont256(pool, sl.record);
        D377_INVARIANT(T, *g, !fe_is_zero(g->z));
        return fe_is_zero(g->z);                              // a record with Z = 0 is no group element: the identity
      }, DCB_WANT_T);
      const ge sum = ge_double_fast(r, true);                 // the chain ran on k / 2: the partial sum is the double
      store_ge_mont256(partials, i, sum);
      if (xyzt_out) store_ge_mont256(xyzt_out, i, sum);
    });
  D377_DCB_END();
}

// ---- one wave per partial sum ---------------------------------------------------------------------------------------------------
// straus_wave_sum<false> (straus_tab.hpp) with every term's point gathered: the workgroup (one wave) sums the slots 0 .. m - 1
// of group q of sum s, m = the group's count (wave-uniform, so no slot is past the end) -> [1/2] of the sum, in every lane.
// An absent slot is walked like a record with Z = 0 -- the identity's table, every digit 0 -- and reads neither point nor scalar.
using row::RQ_WORDS;
__device__ __forceinline__ ge straus_wave_sum_gathered(const SqrtTables& T, const uint64_t* pool, uint32_t pool_count, const int* point_index,
                                                       const uint8_t* scalar32, const LongPlan& plan, size_t s, size_t q, int m,
                                                       uint32_t* tab, uint32_t* xrec, uint32_t (*sdg)[8]) {
  const int t = threadIdx.x;
  const row::RowK K = row::row_consts();
  const row::RowSel S = row::row_sel();
  // points in groups of four: lane t looks after point base + (t & 3) of the group
#pragma unroll 1
  for (int base = 0; base < m; base += 4) {
    const int pj = t & 3;
    const bool mine = base + pj < m;
    const LongSlot sl = long_indexed_slot(plan, s, q, mine ? base + pj : 0, point_index, pool_count);
    ge g = ge_identity();
    bool skip = !mine || sl.kind != SLOT_LIVE;
    if (sl.kind == SLOT_LIVE) {
      g = load_ge_mont256(pool, sl.record);
      skip |= fe_is_zero(g.z);
      D377_INVARIANT(T, g, t < 4 && !skip);
    }
#pragma unroll 1
    for (int j = 0; j < 4 && base + j < m; ++j) {
      const LongSlot sj = long_indexed_slot(plan, s, q, base + j, point_index, pool_count);   // (wave-uniform)
      uint32_t k[8], dg[8];
#pragma unroll
      for (int w = 0; w < 8; ++w) k[w] = 0;
      if (sj.kind == SLOT_LIVE) load32(scalar32, sj.term, k);
      fr_reduce_words(k);
      fr_half_words(k);
      fr_recode_signed16(k, dg);
      if (pj == j && t < 16) row::row_store_from_fe(xrec + 16 * (t >> 2), fe_pick(t >> 2, g.x, g.y, g.z, g.t));
      __syncthreads();
      const bool dead = __shfl((int)skip, j) != 0;                  // (wave-uniform: lane j's verdict on point base + j)
      if (t < 8) sdg[base + j][t] = dead ? 0u : dg[t];              // dead: every digit 0
      row::rq_build_table(dead ? row::rq_identity(S) : xrec[t], tab + (base + j) * row::RQ_TAB_ENTRIES * RQ_WORDS, S, K);
      __syncthreads();
    }
  }
  uint32_t v = row::rq_identity(S);
#pragma unroll 1
  for (int i = 63; i >= 0; --i) {
    if (i != 63) {
#pragma unroll 1
      for (int k = 0; k < 4; ++k) v = row::rq_double_neg(v, S, K);  // four sign-folded doublings keep the sign
    }
#pragma unroll 1
    for (int j = 0; j < m; ++j) {
      const int d = fr_digit(sdg[j], i);
      if (d != 0) v = row::rq_add(v, tab + (j * row::RQ_TAB_ENTRIES + (d < 0 ? -d : d)) * RQ_WORDS, S, d < 0, K);
    }
  }
  __syncthreads();
  xrec[t] = v;
  __syncthreads();
  return row::rq_load_point(xrec);
}

__global__ void __launch_bounds__(64)
k_msm_long_indexed_wave(SqrtTables T, const uint64_t* pool, uint32_t pool_count, const int* point_index, const uint8_t* scalar32,
                        LongPlan plan, size_t np, uint64_t* partials, uint64_t* xyzt_out) {
  extern __shared__ uint32_t tab[];                                // b tables of RQ_TAB_ENTRIES x RQ_WORDS words (dynamic: 2 304 bytes per term)
  __shared__ uint32_t xrec[2 * RQ_WORDS];
  __shared__ uint32_t sdg[BML_GROUP_MAX][8];                       // the points' signed digits (wave-uniform reads in the loop)
  const size_t part = blockIdx.x;                                  // grid = np
  if (part >= np) return;
  const size_t gq = part % plan.g;
  const ge r = straus_wave_sum_gathered(T, pool, pool_count, point_index, scalar32, plan, part / plan.g, gq, (int)plan.count(gq),
                                        tab, xrec, sdg);
  if (threadIdx.x == 0) {
    const ge sum = ge_double_fast(r, true);
    store_ge_mont256(partials, part, sum);
    if (xyzt_out) store_ge_mont256(xyzt_out, part, sum);
  }
}

// ------------------------------------------------------------------------------ host side ---
const char* const HOST = "d377_batch_long_msm_indexed";
const char* const RESIDENT = "d377_batch_long_msm_indexed_resident";

int fail2(int code, const char* fmt, const char* who, size_t a) {
  char msg[320];
  snprintf(msg, sizeof msg, fmt, who, a);
  return fail(code, "%s", msg);
}

// everything on device pointers, enqueued on `s`; the caller holds ctx->mu.  Any m of 1 .. 4096.
int batch_msm_long_indexed_launch(DeviceState& d, hipStream_t s, const uint64_t* pool, uint32_t pool_count, const int* point_index,
                                  const uint8_t* scalars, size_t m, size_t n, uint8_t* out32, uint64_t* xyzt_out) {
  if (n == 0) return D377_OK;
  const SqrtTables T = d.tables();
  const LongPlan plan = long_plan(m);
  const size_t np = n * plan.g;
  uint64_t* direct = plan.g == 1 ? xyzt_out : nullptr;       // no fold level writes the Element records: the chains do
  if (!codec_chunked_ok(d))
    return fail(D377_ERR_INIT, "residency of %s does not match the lane sets of the scratch areas", "k_compress_chunked");
  GuardScope vb{d.vb_guard, s};                              // the lane-set areas, the table scratch, the partials: queue behind their last user
  int rc;
  uint64_t* partials = nullptr;
  if ((rc = long_sums_partials(d, s, n, plan.g, &partials))) return rc;

  // ---- phase 1: the chains, routed as batch_msm_long.hip's: up to four partial sums per SIMD a wave each
  if (np <= sums_wave_max(d)) {                              // (launch_plan.hpp)
    if ((rc = vb.acquire())) return rc;
    const size_t lds = plan.b * row::RQ_TAB_ENTRIES * RQ_WORDS * sizeof(uint32_t);
    hipLaunchKernelGGL(k_msm_long_indexed_wave, dim3((unsigned)np), dim3(64), lds, s, T, pool, pool_count, point_index, scalars, plan, np,
                       partials, direct);
    HIP_TRY(hipGetLastError());
  } else {
    if ((rc = lane_residency(reinterpret_cast<const void*>(k_msm_long_indexed_lane), "k_msm_long_indexed_lane", 0, d.bmli_lds))) return rc;
    uint32_t *tab, *dig;
    if ((rc = straus_scratch_reserve(d, s, plan.b,
           "batch_msm_long_indexed: the table scratch must grow, which cannot happen inside a stream capture",
           "batch_msm_long_indexed: hipMalloc of the table scratch failed (0.23 GB per term of a group on 256 CUs)", &tab, &dig))) return rc;
    if ((rc = vb.acquire())) return rc;
    int grid;
    const DcbScratch dcb = lane_chunks(d, np, &grid);
    hipLaunchKernelGGL(k_msm_long_indexed_lane, dim3((unsigned)grid), dim3(BLOCK), d.bmli_lds, s, T, pool, pool_count, point_index, scalars,
                       plan, np, partials, direct, tab, dig, dcb);
    HIP_TRY(hipGetLastError());
  }

  // ---- phases 2 and 3: the fold levels (none at g = 1), then the sums' Encodings (msm_long_fold.hpp)
  if ((rc = long_sums_fold_compress(d, s, n, plan.g, out32, xyzt_out))) return rc;
  return vb.finish();
}

// the pool's staging area of one device: the host form's alone, grown on demand under ctx->mu
int ensure_pool(DeviceState& d, size_t bytes) { return grow(d.bmli_pool, d.bmli_pool_cap, bytes, bytes / 4 + 4096); }

// one device's slice of a host batch: the WHOLE pool and the slice's indices and scalars in, kernels, copies out, synchronised
int batch_msm_long_indexed_one(DeviceState& d, const uint64_t* pool, size_t pool_count, const int* point_index, const uint8_t* scalars,
                               size_t m, size_t n, uint8_t* out32, uint64_t* xyzt_out) {
  if (n == 0) return D377_OK;
  return device_slice(d, [&]() -> int {
    const size_t terms = n * m;
    int r;
    uint64_t* xyzt_dev;
    if ((r = ensure_pool(d, pool_count * 128))) return r;
    if ((r = ensure(d, 0, terms * sizeof(int)))) return r;
    if ((r = ensure(d, 1, terms * 32))) return r;
    if ((r = sums_out_reserve(d, n, xyzt_out != nullptr, &xyzt_dev))) return r;
    HIP_TRY(hipMemcpyAsync(d.bmli_pool, pool, pool_count * 128, hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d.buf[0], point_index, terms * sizeof(int), hipMemcpyHostToDevice, d.stream));
    HIP_TRY(hipMemcpyAsync(d.buf[1], scalars, terms * 32, hipMemcpyHostToDevice, d.stream));
    if ((r = batch_msm_long_indexed_launch(d, d.stream, reinterpret_cast<const uint64_t*>(d.bmli_pool), (uint32_t)pool_count,
                                           reinterpret_cast<const int*>(d.buf[0]), d.buf[1], m, n, d.buf[2], xyzt_dev))) return r;
    return sums_out_copy(d, n, out32, xyzt_out);
  });
}

// What both forms check first, in the documented order and before any device is touched: m, pool_count, null buffers when
// n > 0, ctx.
int check_args(const char* who, d377_ctx* ctx, const uint64_t* pool, size_t pool_count, const int* point_index, const uint8_t* scalars,
               size_t m, size_t n, const uint8_t* out32) {
  if (m < 1 || m > BMLI_MAX)
    return fail2(D377_ERR_ARG, "%s: m = %zu: 1 .. 4096 terms per sum (D377_BATCH_MSM_LONG_MAX_TERMS); d377_msm for longer sums", who, m);
  if (pool_count < 1 || pool_count > BMLI_POOL_MAX)
    return fail2(D377_ERR_ARG, "%s: pool_count = %zu: the pool holds 1 .. 2^31 - 1 Element records", who, pool_count);
  if (n) {
    if (!pool) return fail(D377_ERR_ARG, "%s: null buffer: pool_xyzt", who);
    if (!point_index) return fail(D377_ERR_ARG, "%s: null buffer: point_index", who);
    if (!scalars) return fail(D377_ERR_ARG, "%s: null buffer: scalar32", who);
    if (!out32) return fail(D377_ERR_ARG, "%s: null buffer: enc32_out", who);
  }
  if (!ctx) return fail(D377_ERR_ARG, "%s: null context: ctx", who);
  if (n > SIZE_MAX / 32 / m) return fail(D377_ERR_ARG, "%s: n x m overflows", who);
  return D377_OK;
}

}  // namespace

extern "C" {

// host pointers: every index is read before any copy or launch, so no kernel sees one the host form refuses
int d377_batch_long_msm_indexed(d377_ctx* ctx, const uint64_t* pool_xyzt, size_t pool_count, const int* point_index,
                                const uint8_t* scalar32, size_t m, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out) {
  int rc;
  if ((rc = check_args(HOST, ctx, pool_xyzt, pool_count, point_index, scalar32, m, n, enc32_out))) return rc;
  if (n == 0) return D377_OK;
  const size_t terms = n * m;
  for (size_t p = 0; p < terms; ++p) {
    const int b = point_index[p];
    if (b != -1 && !pool_index_live(b, (uint32_t)pool_count)) {
      snprintf(d377_g_err, sizeof d377_g_err,
               "%s: point_index[%zu] = %d (sum %zu, term %zu) is neither -1 nor a record 0 .. %zu of the pool", HOST, p, b, p / m, p % m,
               pool_count - 1);
      return D377_ERR_ARG;
    }
  }
  std::lock_guard<std::mutex> lock(ctx->mu);
  // contiguous slices of the SUMS over the context's devices; the pool goes to every device that gets a slice
  return slice_over_devices(ctx, n, [&](size_t k, size_t lo, size_t cnt) {
    return batch_msm_long_indexed_one(ctx->devs[k], pool_xyzt, pool_count, point_index + lo * m, scalar32 + lo * m * 32, m, cnt,
                                      enc32_out + lo * 32, xyzt_out ? xyzt_out + lo * 16 : nullptr);
  });
}

// The indices are not read on the host: the verdict kernel counts the refused ones in front of the chains, whose unsigned
// compare walks a refused index as an absent term (batch_msm_long_indexed_plan.hpp).
int d377_batch_long_msm_indexed_resident(d377_ctx* ctx, int dev, void* stream, const uint64_t* pool_xyzt, size_t pool_count,
                                         const int* point_index, const uint8_t* scalar32, size_t m, size_t n, uint8_t* enc32_out,
                                         uint64_t* xyzt_out, uint64_t* verdict) {
  int rc;
  if ((rc = check_args(RESIDENT, ctx, pool_xyzt, pool_count, point_index, scalar32, m, n, enc32_out))) return rc;
  if (dev < 0 || (size_t)dev >= ctx->devs.size()) return fail(D377_ERR_ARG, "%s: dev is not a device of this context", RESIDENT);
  if (!aligned16(pool_xyzt) || !aligned16(scalar32) || !aligned16(enc32_out) || !aligned16(xyzt_out))
    return fail(D377_ERR_ARG, "%s: device record buffers must be 16-byte aligned", RESIDENT);
  if (!aligned_to(point_index, 4)) return fail(D377_ERR_ARG, "%s: point_index must be 4-byte aligned", RESIDENT);
  if (!aligned_to(verdict, 8)) return fail(D377_ERR_ARG, "%s: verdict must be 8-byte aligned", RESIDENT);
  if (n == 0) return D377_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceState& d = ctx->devs[(size_t)dev];
  HIP_TRY(hipSetDevice(d.id));
  if (verdict && (rc = index_verdict_launch(d, (hipStream_t)stream, point_index, n * m, (int)pool_count, verdict))) return rc;
  return batch_msm_long_indexed_launch(d, (hipStream_t)stream, pool_xyzt, (uint32_t)pool_count, point_index, scalar32, m, n, enc32_out,
                                       xyzt_out);
}

}  // extern "C"
