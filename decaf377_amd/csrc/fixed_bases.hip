// fixed_bases.hip -- fixed-base combs for caller-chosen points and many sums over them (gfx950):
//   d377_fixed_bases_create   one comb per base on every device (fixed_comb.hpp: k_fb_window_bases, then ONE k_init_fbase
//                             launch over the m x W windows of all bases)
//   d377_batch_fixed_msm      out[i] = sum_j scalar[i m + j] * B_j, one lane per sum
//   d377_batch_fixed_msm_indexed   out[i] = sum_{j < t} scalar[i t + j] * B_{base_index[i t + j]}: the same walk, each term in
//                             the comb it names (curve.hpp: ge_fixed_msm_indexed_w8); -1 = the term is absent
//   d377_fixed_bases_create_long   the same registration for up to D377_FIXED_BASES_LONG_MAX = 4096 bases
//   d377_batch_fixed_long_msm      the dense sums with every sum cut into g segments of consecutive bases
//                             (fixed_msm_long_plan.hpp), one lane per segment (k_fixed_msm_seg); the segments' partial sums are
//                             folded and compressed as d377_batch_msm_long's are (msm_long_fold.hpp).  g = 1: the kernel above
//   d377_batch_fixed_*_resident    the three kinds of sums on device pointers and a stream: the same launchers without the
//                             staging frame.  The indexed form does not read its indices on the host: k_index_verdict
//                             (index_verdict.hpp) writes one record per call, and d377_check_base_index_resident runs it alone
//
// The sum is k_scalar_mul_base's walk widened to m combs (curve.hpp: ge_fixed_msm_w8): each base's scalar is reduced and
// halved, its W signed digits pick one entry per window, and all m x W mixed additions go into ONE accumulator -- no
// doubling anywhere.  The walk yields H = sum_j (k_j / 2 mod r) B_j, and the encoding of 2 H comes out of the square-root-free
// compressor (ge_dcb_from_half), its inversion shared with the chunk's other sums (dcb.hpp), as for the generator comb.
// Against d377_batch_msm_small's Straus chain (252 doublings + 64 m additions + m window tables per sum) this is 14-32 mixed
// additions per base and nothing else.
//
// A translation unit of its own, like batch_msm.hip: the register tables of d377.hip's kernels are measured artefacts.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/decaf377_amd.h"
#include "curve.hpp"
#include "device_util.hpp"
#include "dcb.hpp"
#include "host_state.hpp"
#include "batch_host.hpp"
#include "fixed_comb.hpp"
#include "comb_tabs.hpp"
#include "codec_chunked.hpp"
#include "fixed_msm_long_plan.hpp"
#include "msm_long_fold.hpp"
#include "index_verdict.hpp"

using namespace d377;

namespace {

constexpr int FX_MAX = D377_FIXED_BASES_MAX;
constexpr int FX_LONG_MAX = D377_FIXED_BASES_LONG_MAX;
static_assert(FX_LONG_MAX <= 4096, "g <= m segments must fold in three levels of BML_FOLD = 16");

// One lane per sum, in chunks like k_scalar_mul_base (dcb.hpp): the sums of a chunk share one inversion per wave.  No table
// scratch -- the combs are the handle's -- so the lane sets are only the round records.
template <int BITS>
__global__ void __launch_bounds__(BLOCK, WAVES_PER_SIMD)
k_fixed_msm_lane(SqrtTables T, const uint32_t* tabs, const uint8_t* scalar32, int m, size_t n, uint8_t* out32, uint64_t* xyzt_out,
                 DcbScratch dcb) {
  __shared__ uint32_t lds_pow_[1];                                 // (no square root here: residency is set by the launch's padding)
  LdsPowTab pt;
  pt.col = lds_pow_;
  D377_DCB_BEGIN(out32);
  const CombTabs<BITS> ft{tabs};
  dcb_rounds<0, true>(n, io, pt,
    [&](size_t, int) {},
    [&](size_t i, int j, const uint32_t (*)[8], bool) {
      const size_t first = i * (size_t)m;
      const ge r = ge_fixed_msm_w8<BITS>(m, [&](int p, uint32_t k[8]) {
        load32(scalar32, first + (size_t)p, k);
        fr_reduce_words(k);
        fr_half_words(k);                                          // the walk yields H = sum (k / 2) B: the encoding of 2 H needs no root
      }, ft, DCB_WANT_T);
      D377_INVARIANT(T, r, true);
      if (xyzt_out) store_ge_mont256(xyzt_out, i, ge_double_fast(r, true));   // the sum itself is the double
      dcb_put(io, j, ge_dcb_from_half(r, false));
    });
  D377_DCB_END();
}

// The sum whose terms name their bases: term p of lane i walks comb base_index[i t + p].  The lanes of a wave gather from
// different combs; their control flow is the dense kernel's.  An absent term (-1) walks scalar 0 on comb 0, entry 0 of every
// window, the identity record.  The host form has refused every other index outside 0 .. m-1 before the launch
// (d377_batch_fixed_msm_indexed); the resident form has not read them, and its contract is what the unsigned compare below
// does: such an index is walked as an absent term, so no index can address past the m combs (k_index_verdict counts them).
template <int BITS>
__global__ void __launch_bounds__(BLOCK, WAVES_PER_SIMD)
k_fixed_msm_indexed_lane(SqrtTables T, const uint32_t* tabs, const int* base_index, const uint8_t* scalar32, int m, int t, size_t n,
                         uint8_t* out32, uint64_t* xyzt_out, DcbScratch dcb) {
  __shared__ uint32_t lds_pow_[1];                                 // (no square root here: residency is set by the launch's padding)
  LdsPowTab pt;
  pt.col = lds_pow_;
  D377_DCB_BEGIN(out32);
  const CombTabs<BITS> ft{tabs};
  dcb_rounds<0, true>(n, io, pt,
    [&](size_t, int) {},
    [&](size_t i, int j, const uint32_t (*)[8], bool) {
      const size_t first = i * (size_t)t;
      const ge r = ge_fixed_msm_indexed_w8<BITS>(t, [&](int p, uint32_t k[8]) -> int {
        const int b = base_index[first + (size_t)p];               // once per term
        load32(scalar32, first + (size_t)p, k);
        fr_reduce_words(k);
        fr_half_words(k);
        const uint32_t keep = (uint32_t)b < (uint32_t)m ? ~0u : 0u;
#pragma unroll
        for (int q = 0; q < 8; ++q) k[q] &= keep;
        return (int)((uint32_t)b & keep);
      }, ft, DCB_WANT_T);
      D377_INVARIANT(T, r, true);
      if (xyzt_out) store_ge_mont256(xyzt_out, i, ge_double_fast(r, true));   // the sum itself is the double
      dcb_put(io, j, ge_dcb_from_half(r, false));
    });
  D377_DCB_END();
}

// The dense sum cut into segments (fixed_msm_long_plan.hpp): one lane per PARTIAL sum, a plain grid-stride kernel.  No table
// scratch and no inversion, so it claims no lane set and cannot starve.  Lane P takes segment q = P / n of sum s = P % n --
// segment-major, so the lanes of a wave gather from the SAME combs and few combs are in flight chip-wide at any moment -- and
// writes record s g + q, sum-major, because the fold adds consecutive records of a sum.  The record is the double of the
// walk's result (the walk ran on k / 2), what k_msm_long_lane writes.  (-DD377_FML_SUM_MAJOR: the A/B build with sum-major lanes.)
template <class FTab>
struct FbOffsetTabs {
  const FTab& tabs;
  int first;                                                       // the segment's first base
  __device__ __forceinline__ gea load(int j, int i, int c, bool swap) const { return tabs.load(first + j, i, c, swap); }
};
template <int BITS>
__global__ void __launch_bounds__(BLOCK, WAVES_PER_SIMD)
k_fixed_msm_seg(SqrtTables T, const uint32_t* tabs, const uint8_t* scalar32, FixedLongPlan plan, size_t n, uint64_t* partials) {
  const CombTabs<BITS> ft{tabs};
  const size_t total = n * plan.g;
#pragma unroll 1
  for (size_t P = (size_t)blockIdx.x * BLOCK + threadIdx.x; P < total; P += (size_t)gridDim.x * BLOCK) {
#ifdef D377_FML_SUM_MAJOR
    const size_t s = P / plan.g, q = P % plan.g;
#else
    const size_t q = P / n, s = P % n;
#endif
    const size_t first = s * plan.m + plan.first(q);
    const FbOffsetTabs<CombTabs<BITS>> st{ft, (int)plan.first(q)};
    const ge r = ge_fixed_msm_w8<BITS>((int)plan.count(q), [&](int p, uint32_t k[8]) {
      load32(scalar32, first + (size_t)p, k);
      fr_reduce_words(k);
      fr_half_words(k);
    }, st, /*want_t=*/false);
    const ge sum = ge_double_fast(r, true);
    D377_INVARIANT(T, sum, true);
    store_ge_mont256(partials, s * plan.g + q, sum);
  }
}

// The verdict on a resident call's indices (index_verdict.hpp): a grid-stride pass over `count` ints.  Every lane joins the
// verdicts of its entries, the lanes of a wave join theirs by butterfly shuffles, and lane 0 of a wave that found an
// offender adds its count to verdict[0] and lowers verdict[1] to its first position: at most one atomic of each kind per
// wave, none for a clean array.  k_index_verdict_init writes the record (0, none) in front of it on the same stream.
__global__ void k_index_verdict_init(uint64_t* verdict) {
  if (threadIdx.x == 0) verdict[0] = 0;
  if (threadIdx.x == 1) verdict[1] = INDEX_VERDICT_NONE;
}
__global__ void __launch_bounds__(BLOCK) k_index_verdict(const int* base_index, size_t count, int m, uint64_t* verdict) {
  static_assert(BLOCK % 64 == 0, "whole waves: every lane takes part in the shuffles");
  IndexVerdict v = verdict_none();
  for (size_t p = (size_t)blockIdx.x * BLOCK + threadIdx.x; p < count; p += (size_t)gridDim.x * BLOCK)
    v = verdict_join(v, verdict_of(base_index[p], m, (uint64_t)p));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const IndexVerdict o{(uint64_t)__shfl_xor((unsigned long long)v.count, off, 64), (uint64_t)__shfl_xor((unsigned long long)v.first, off, 64)};
    v = verdict_join(v, o);
  }
  if ((threadIdx.x & 63) == 0 && v.count != 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(verdict), (unsigned long long)v.count);
    atomicMin(reinterpret_cast<unsigned long long*>(verdict) + 1, (unsigned long long)v.first);
  }
}

// ------------------------------------------------------------------------------ host side ---
// what with_width (comb_tabs.hpp) says to a width no registration can have
constexpr const char* WIDTH_REFUSAL = "d377_fixed_bases_create: comb_bits must be 8, 12, 16 or 18 (0 = 16)";
template <int BITS>
size_t comb_bytes() { return (size_t)FbShape<BITS>::windows * FbShape<BITS>::entries * FBW_ENTRY_WORDS * sizeof(uint32_t); }

// Residency of the two lane kernels against the lane sets (batch_host.hpp), once per device and width, by
// d377_fixed_bases_create; the caller holds ctx->mu.
template <int BITS>
int check_residency_fx(DeviceState& d) {
  int rc = lane_residency(reinterpret_cast<const void*>(k_fixed_msm_lane<BITS>), "k_fixed_msm_lane", BITS, d.fx_lds[width_slot(BITS)]);
  if (rc) return rc;
  return lane_residency(reinterpret_cast<const void*>(k_fixed_msm_indexed_lane<BITS>), "k_fixed_msm_indexed_lane", BITS,
                        d.fxi_lds[width_slot(BITS)]);
}

// the combs of `m` bases on one device: residency check, allocation, window bases, one build launch, synchronised.
// On failure nothing of this device is left allocated.  Caller holds ctx->mu.
template <int BITS>
int build_on(DeviceState& d, const char* who, const uint64_t* xyzt, size_t m, uint32_t** out) {
  using Sh = FbShape<BITS>;
  *out = nullptr;
  HIP_TRY(hipSetDevice(d.id));
  int rc = check_residency_fx<BITS>(d);
  if (rc) return rc;
  const size_t bytes = m * comb_bytes<BITS>(), nwin = m * (size_t)Sh::windows;
  uint32_t* tab = nullptr;
  uint64_t* rec = nullptr;
  uint32_t* wb = nullptr;
  auto cleanup = [&]() { (void)hipFree(tab); (void)hipFree(rec); (void)hipFree(wb); };
  if (hipMalloc(&tab, bytes) != hipSuccess) {
    (void)hipGetLastError();
    tab = nullptr;
    snprintf(d377_g_err, sizeof d377_g_err,
             "%s: the combs need %.3f GB of device memory and the allocation failed (device %d): fewer bases or a "
             "narrower comb_bits", who, (double)bytes / 1e9, d.id);
    return D377_ERR_HIP;
  }
  if (hipMalloc(&rec, m * 16 * sizeof(uint64_t)) != hipSuccess || hipMalloc(&wb, nwin * 4 * SLOT * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();
    cleanup();
    return fail(D377_ERR_HIP, "%s: hipMalloc failed (window bases)", who);
  }
  hipError_t e = hipMemcpyAsync(rec, xyzt, m * 16 * sizeof(uint64_t), hipMemcpyHostToDevice, d.stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_fb_window_bases<BITS>, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, d.stream, rec, (int)m, wb);
    const size_t runs = nwin * ((Sh::entries + FB_RUN - 1) / FB_RUN);
    hipLaunchKernelGGL(k_init_fbase<BITS>, dim3((unsigned)((runs + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, d.stream, wb, tab, nwin);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(d.stream);
  (void)hipFree(rec); rec = nullptr;
  (void)hipFree(wb); wb = nullptr;
  if (e != hipSuccess) {
    cleanup();
    snprintf(d377_g_err, sizeof d377_g_err, "%s: building the combs: %s", who, hipGetErrorString(e));
    return D377_ERR_HIP;
  }
  *out = tab;
  return D377_OK;
}

// everything on device pointers, enqueued on `s`; the caller holds ctx->mu.  index == null: the dense sums over all m bases;
// otherwise n x t indices the host has checked, and t terms per sum.
int fixed_msm_launch(DeviceState& d, hipStream_t s, const FixedBases& fb, const uint32_t* tab, const int* index, size_t t,
                     const uint8_t* scalars, size_t n, uint8_t* out32, uint64_t* xyzt_out) {
  if (n == 0) return D377_OK;
  const int lds = index ? d.fxi_lds[width_slot(fb.bits)] : d.fx_lds[width_slot(fb.bits)];
  if (lds < 0) return fail(D377_ERR_INIT, "%s: residency not checked on this device", index ? "k_fixed_msm_indexed_lane" : "k_fixed_msm_lane");
  GuardScope vb{d.vb_guard, s};                              // the lane-set areas: queue behind their last user
  int rc;
  if ((rc = vb.acquire())) return rc;
  int grid;
  const DcbScratch dcb = lane_chunks(d, n, &grid);
  const SqrtTables T = d.tables();
  if ((rc = with_width(fb.bits, WIDTH_REFUSAL, [&](auto b) -> int {
         if (index)
           hipLaunchKernelGGL(k_fixed_msm_indexed_lane<decltype(b)::value>, dim3((unsigned)grid), dim3(BLOCK), lds, s, T, tab,
                              index, scalars, (int)fb.m, (int)t, n, out32, xyzt_out, dcb);
         else
           hipLaunchKernelGGL(k_fixed_msm_lane<decltype(b)::value>, dim3((unsigned)grid), dim3(BLOCK), lds, s, T, tab, scalars,
                              (int)fb.m, n, out32, xyzt_out, dcb);
         return D377_OK; }))) return rc;
  HIP_TRY(hipGetLastError());
  return vb.finish();
}

// the cut of n dense sums on device d (n >= 1)
FixedLongPlan cut_of(const DeviceState& d, const FixedBases& fb, size_t n) { return fixed_long_plan(fb.m, n, d.resident_lanes()); }

// The dense sums cut into segments; everything on device pointers, enqueued on `s`; the caller holds ctx->mu.  One segment per
// sum is fixed_msm_launch, the same bytes.
int fixed_msm_long_launch(DeviceState& d, hipStream_t s, const FixedBases& fb, const uint32_t* tab, const uint8_t* scalars, size_t n,
                          uint8_t* out32, uint64_t* xyzt_out) {
  if (n == 0) return D377_OK;
  const FixedLongPlan plan = cut_of(d, fb, n);
  if (plan.g == 1) return fixed_msm_launch(d, s, fb, tab, nullptr, fb.m, scalars, n, out32, xyzt_out);
  if (!codec_chunked_ok(d))
    return fail(D377_ERR_INIT, "residency of %s does not match the lane sets of the scratch areas", "k_compress_chunked");
  GuardScope vb{d.vb_guard, s};                              // the partials and, for the compressor, the lane-set areas
  int rc;
  uint64_t* partials = nullptr;
  if ((rc = long_sums_partials(d, s, n, plan.g, &partials))) return rc;
  if ((rc = vb.acquire())) return rc;
  const int grid = fold_grid(d, n * plan.g);
  const SqrtTables T = d.tables();
  if ((rc = with_width(fb.bits, WIDTH_REFUSAL, [&](auto b) -> int {
         hipLaunchKernelGGL(k_fixed_msm_seg<decltype(b)::value>, dim3((unsigned)grid), dim3(BLOCK), 0, s, T, tab, scalars, plan, n, partials);
         return D377_OK; }))) return rc;
  HIP_TRY(hipGetLastError());
  if ((rc = long_sums_fold_compress(d, s, n, plan.g, out32, xyzt_out))) return rc;
  return vb.finish();
}

// one device's slice of a host batch: copies in, kernel, copies out, synchronised.  index == null: dense, t = m; otherwise the
// slice's n x t indices, staged behind its scalars (n t x 32 bytes: 16-byte aligned).  cut: the dense sums in segments.
int fixed_msm_one(DeviceState& d, const FixedBases& fb, const uint32_t* tab, const int* index, size_t t, bool cut, const uint8_t* scalars,
                  size_t n, uint8_t* out32, uint64_t* xyzt_out) {
  if (n == 0) return D377_OK;
  return device_slice(d, [&]() -> int {
    const size_t terms = n * t;
    int r;
    uint64_t* xyzt_dev;
    if ((r = ensure(d, 1, terms * 32 + (index ? terms * sizeof(int) : 0)))) return r;
    if ((r = sums_out_reserve(d, n, xyzt_out != nullptr, &xyzt_dev))) return r;
    HIP_TRY(hipMemcpyAsync(d.buf[1], scalars, terms * 32, hipMemcpyHostToDevice, d.stream));
    const int* index_dev = index ? reinterpret_cast<const int*>(d.buf[1] + terms * 32) : nullptr;
    if (index) HIP_TRY(hipMemcpyAsync(d.buf[1] + terms * 32, index, terms * sizeof(int), hipMemcpyHostToDevice, d.stream));
    if (cut) r = fixed_msm_long_launch(d, d.stream, fb, tab, d.buf[1], n, d.buf[2], xyzt_dev);
    else r = fixed_msm_launch(d, d.stream, fb, tab, index_dev, t, d.buf[1], n, d.buf[2], xyzt_dev);
    if (r) return r;
    return sums_out_copy(d, n, out32, xyzt_out);
  });
}

// n sums in contiguous slices over the context's devices (host_state.hpp: slice_over_devices); t terms per sum,
// index == null for the dense sums, which `cut` has every device cut into segments.  Caller holds ctx->mu.
int fixed_msm_sliced(d377_ctx* ctx, const FixedBases& fb, const int* index, size_t t, bool cut, const uint8_t* scalar32, size_t n,
                     uint8_t* enc32_out, uint64_t* xyzt_out) {
  if (n == 0) return D377_OK;
  return slice_over_devices(ctx, n, [&](size_t k, size_t lo, size_t cnt) {
    return fixed_msm_one(ctx->devs[k], fb, fb.tab[k], index ? index + lo * t : nullptr, t, cut, scalar32 + lo * t * 32, cnt,
                         enc32_out + lo * 32, xyzt_out ? xyzt_out + lo * 16 : nullptr);
  });
}

// frees a registration's tables (every device); caller holds ctx->mu or is destroying the context
void free_tables(d377_ctx* ctx, FixedBases* fb) {
  for (size_t k = 0; k < fb->tab.size(); ++k) {
    if (!fb->tab[k]) continue;
    DeviceState& d = ctx->devs[k];
    (void)hipSetDevice(d.id);
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    (void)d.vb_guard.drain();                                // a launch on the table may be in flight on another stream
    (void)hipFree(fb->tab[k]);
    fb->tab[k] = nullptr;
  }
}

// the live registration `handle` of the context, or null; caller holds ctx->mu
FixedBases* find(d377_ctx* ctx, int64_t handle) {
  for (FixedBases* fb : ctx->fixed)
    if (fb->handle == handle) return fb;
  return nullptr;
}

// the registration itself, arguments checked: the combs on every device, then the handle.  On failure nothing is left allocated.
int register_bases(d377_ctx* ctx, const char* who, const uint64_t* xyzt, size_t m, int bits, int64_t* handle_out) {
  std::lock_guard<std::mutex> lock(ctx->mu);
  FixedBases* fb = new (std::nothrow) FixedBases;
  if (!fb) return fail(D377_ERR_ARG, "%s: out of host memory", who);
  fb->m = m;
  fb->bits = bits;
  fb->tab.assign(ctx->devs.size(), nullptr);
  int rc = with_width(bits, WIDTH_REFUSAL, [&](auto b) -> int {
    constexpr int BITS = decltype(b)::value;
    fb->bytes = (uint64_t)(m * comb_bytes<BITS>());
    for (size_t k = 0; k < ctx->devs.size(); ++k) {
      const int r = build_on<BITS>(ctx->devs[k], who, xyzt, m, &fb->tab[k]);
      if (r) return r;
    }
    return D377_OK;
  });
  if (rc) {
    char saved[sizeof d377_g_err];
    memcpy(saved, d377_g_err, sizeof saved);
    free_tables(ctx, fb);
    delete fb;
    memcpy(d377_g_err, saved, sizeof saved);
    return rc;
  }
  fb->handle = ctx->next_fixed++;
  ctx->fixed.push_back(fb);
  *handle_out = fb->handle;
  return D377_OK;
}

}  // namespace

namespace d377 {
void fixed_bases_release_all(d377_ctx* ctx) {
  for (FixedBases* fb : ctx->fixed) {
    free_tables(ctx, fb);
    delete fb;
  }
  ctx->fixed.clear();
}
FixedBases* fixed_bases_find(d377_ctx* ctx, int64_t handle) { return find(ctx, handle); }

// No scratch and no lane set: nothing to guard, and nothing that could starve.
int index_verdict_launch(DeviceState& d, hipStream_t s, const int* base_index, size_t count, int m, uint64_t* verdict) {
  hipLaunchKernelGGL(k_index_verdict_init, dim3(1), dim3(64), 0, s, verdict);
  HIP_TRY(hipGetLastError());
  if (count == 0) return D377_OK;
  hipLaunchKernelGGL(k_index_verdict, dim3((unsigned)fold_grid(d, count)), dim3(BLOCK), 0, s, base_index, count, m, verdict);
  HIP_TRY(hipGetLastError());
  return D377_OK;
}
}  // namespace d377

namespace {

// the dense sums on device pointers; cut: every sum in segments (a handle of more than 64 bases is always cut, as on the host)
int fixed_msm_resident(const char* who, d377_ctx* ctx, int dev, void* stream, int64_t handle, bool cut, const uint8_t* scalar32,
                       size_t n, uint8_t* enc32_out, uint64_t* xyzt_out) {
  if (!ctx) return fail(D377_ERR_ARG, "%s: ctx is null", who);
  if (n && (!scalar32 || !enc32_out)) return fail(D377_ERR_ARG, "%s: null buffer", who);
  std::lock_guard<std::mutex> lock(ctx->mu);
  ResidentCall c;
  const void* rec[3] = {scalar32, enc32_out, xyzt_out};
  int rc;
  if ((rc = resident_enter(who, ctx, dev, handle, rec, 3, nullptr, nullptr, &c))) return rc;
  if (n > SIZE_MAX / 32 / c.fb->m) return fail(D377_ERR_ARG, "%s: n x m overflows", who);
  if (cut || c.fb->m > (size_t)FX_MAX)
    return fixed_msm_long_launch(*c.d, (hipStream_t)stream, *c.fb, c.tab, scalar32, n, enc32_out, xyzt_out);
  return fixed_msm_launch(*c.d, (hipStream_t)stream, *c.fb, c.tab, nullptr, c.fb->m, scalar32, n, enc32_out, xyzt_out);
}

}  // namespace

extern "C" {

int d377_fixed_bases_create(d377_ctx* ctx, const uint64_t* xyzt, size_t m, int comb_bits, int64_t* handle_out) {
  if (handle_out) *handle_out = 0;
  if (m < 1 || m > (size_t)FX_MAX)
    return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_create: m must be 1 .. 64 bases (D377_FIXED_BASES_MAX)");
  const int bits = comb_bits == 0 ? 16 : comb_bits;
  if (width_slot(bits) < 0) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_create: comb_bits must be 8, 12, 16 or 18 (0 = 16)");
  if (!xyzt) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_create: xyzt is null");
  if (!handle_out) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_create: handle_out is null");
  if (!ctx) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_create: ctx is null");
  return register_bases(ctx, "d377_fixed_bases_create", xyzt, m, bits, handle_out);
}

// the same registration with room for 4096 bases; nothing in the comb layout depends on the count (fixed_comb.hpp)
int d377_fixed_bases_create_long(d377_ctx* ctx, const uint64_t* xyzt, size_t m, int comb_bits, int64_t* handle_out) {
  if (handle_out) *handle_out = 0;
  if (m < 1 || m > (size_t)FX_LONG_MAX)
    return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_create_long: m must be 1 .. 4096 bases (D377_FIXED_BASES_LONG_MAX)");
  const int bits = comb_bits == 0 ? 12 : comb_bits;
  if (width_slot(bits) < 0) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_create_long: comb_bits must be 8, 12, 16 or 18 (0 = 12)");
  if (!xyzt) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_create_long: xyzt is null");
  if (!handle_out) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_create_long: handle_out is null");
  if (!ctx) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_create_long: ctx is null");
  return register_bases(ctx, "d377_fixed_bases_create_long", xyzt, m, bits, handle_out);
}

int d377_fixed_bases_info(d377_ctx* ctx, int64_t handle, uint64_t* m, int* comb_bits, uint64_t* table_bytes_per_device) {
  if (!ctx) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_info: ctx is null");
  std::lock_guard<std::mutex> lock(ctx->mu);
  const FixedBases* fb = find(ctx, handle);
  if (!fb) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_info: handle is not a live registration of this context");
  if (m) *m = fb->m;
  if (comb_bits) *comb_bits = fb->bits;
  if (table_bytes_per_device) *table_bytes_per_device = fb->bytes;
  return D377_OK;
}

int d377_fixed_bases_destroy(d377_ctx* ctx, int64_t handle) {
  if (!ctx) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_destroy: ctx is null");
  std::lock_guard<std::mutex> lock(ctx->mu);
  FixedBases* fb = find(ctx, handle);
  if (!fb) return fail(D377_ERR_ARG, "%s", "d377_fixed_bases_destroy: handle is not a live registration of this context");
  ctx->fixed.erase(std::find(ctx->fixed.begin(), ctx->fixed.end(), fb));
  free_tables(ctx, fb);
  delete fb;
  return D377_OK;
}

// host pointers: contiguous slices of the SUMS over the context's devices
int d377_batch_fixed_msm(d377_ctx* ctx, int64_t handle, const uint8_t* scalar32, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out) {
  if (!ctx) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_msm: ctx is null");
  if (n && (!scalar32 || !enc32_out)) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_msm: null buffer");
  std::lock_guard<std::mutex> lock(ctx->mu);
  const FixedBases* fb = find(ctx, handle);
  if (!fb) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_msm: handle is not a live registration of this context");
  // more bases than d377_fixed_bases_create registers: the same sum, cut into segments (d377_batch_fixed_long_msm)
  return fixed_msm_sliced(ctx, *fb, nullptr, fb->m, fb->m > (size_t)FX_MAX, scalar32, n, enc32_out, xyzt_out);
}

// the same slices; the index rows and scalar rows of a sum travel with it
int d377_batch_fixed_msm_indexed(d377_ctx* ctx, int64_t handle, const int* base_index, const uint8_t* scalar32, size_t t, size_t n,
                                 uint8_t* enc32_out, uint64_t* xyzt_out) {
  if (t < 1 || t > (size_t)FX_MAX)
    return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_msm_indexed: t must be 1 .. 64 terms per sum (D377_FIXED_BASES_MAX)");
  if (n && !base_index) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_msm_indexed: base_index is null");
  if (n && !scalar32) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_msm_indexed: scalar32 is null");
  if (n && !enc32_out) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_msm_indexed: enc32_out is null");
  if (!ctx) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_msm_indexed: ctx is null");
  std::lock_guard<std::mutex> lock(ctx->mu);
  const FixedBases* fb = find(ctx, handle);
  if (!fb) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_msm_indexed: handle is not a live registration of this context");
  if (n > SIZE_MAX / 32 / t) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_msm_indexed: n x t overflows");
  // every index, before any copy or launch: no kernel sees one it could read out of bounds with
  const size_t terms = n * t;
  const int m = (int)fb->m;
  for (size_t p = 0; p < terms; ++p) {
    const int b = base_index[p];
    if (b < -1 || b >= m) {
      snprintf(d377_g_err, sizeof d377_g_err,
               "d377_batch_fixed_msm_indexed: base_index[%zu] = %d (sum %zu, term %zu) is neither -1 nor a base 0 .. %d of this registration",
               p, b, p / t, p % t, m - 1);
      return D377_ERR_ARG;
    }
  }
  return fixed_msm_sliced(ctx, *fb, base_index, t, false, scalar32, n, enc32_out, xyzt_out);
}

// the dense sums, every sum cut into segments where that fills the chip; any live handle
int d377_batch_fixed_long_msm(d377_ctx* ctx, int64_t handle, const uint8_t* scalar32, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out) {
  if (!ctx) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_long_msm: ctx is null");
  if (n && (!scalar32 || !enc32_out)) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_long_msm: null buffer");
  std::lock_guard<std::mutex> lock(ctx->mu);
  const FixedBases* fb = find(ctx, handle);
  if (!fb) return fail(D377_ERR_ARG, "%s", "d377_batch_fixed_long_msm: handle is not a live registration of this context");
  return fixed_msm_sliced(ctx, *fb, nullptr, fb->m, true, scalar32, n, enc32_out, xyzt_out);
}

// how device `dev` of the context cuts its slice of a call of n sums (fixed_msm_sliced: ceil(n / devices) sums per device)
int d377_fixed_long_msm_plan(d377_ctx* ctx, int64_t handle, size_t n, int dev, uint64_t* segments, uint64_t* bases_per_segment) {
  if (segments) *segments = 0;
  if (bases_per_segment) *bases_per_segment = 0;
  if (!ctx) return fail(D377_ERR_ARG, "%s", "d377_fixed_long_msm_plan: ctx is null");
  std::lock_guard<std::mutex> lock(ctx->mu);
  const FixedBases* fb = find(ctx, handle);
  if (!fb) return fail(D377_ERR_ARG, "%s", "d377_fixed_long_msm_plan: handle is not a live registration of this context");
  const size_t nd = ctx->devs.size();
  if (dev < 0 || (size_t)dev >= nd) return fail(D377_ERR_ARG, "%s", "d377_fixed_long_msm_plan: dev is not a device of this context");
  const size_t per = (n + nd - 1) / nd, lo = per * (size_t)dev;
  const size_t cnt = lo >= n ? 0 : (lo + per <= n ? per : n - lo);
  if (cnt == 0) return D377_OK;                               // no sums for this device: 0 segments
  const FixedLongPlan plan = cut_of(ctx->devs[(size_t)dev], *fb, cnt);
  if (segments) *segments = plan.g;
  if (bases_per_segment) *bases_per_segment = plan.b;
  return D377_OK;
}

// ---- the resident forms: device pointers, enqueued on `stream`, no host synchronisation (include/decaf377_amd.h)
int d377_batch_fixed_msm_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const uint8_t* scalar32, size_t n,
                                  uint8_t* enc32_out, uint64_t* xyzt_out) {
  return fixed_msm_resident("d377_batch_fixed_msm_resident", ctx, dev, stream, handle, false, scalar32, n, enc32_out, xyzt_out);
}
int d377_batch_fixed_long_msm_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const uint8_t* scalar32, size_t n,
                                       uint8_t* enc32_out, uint64_t* xyzt_out) {
  return fixed_msm_resident("d377_batch_fixed_long_msm_resident", ctx, dev, stream, handle, true, scalar32, n, enc32_out, xyzt_out);
}

// The indices are not read on the host: the verdict kernel counts the refused ones in front of the sums kernel, whose
// unsigned compare walks a refused index as an absent term.
int d377_batch_fixed_msm_indexed_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const int* base_index,
                                          const uint8_t* scalar32, size_t t, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out,
                                          uint64_t* verdict) {
  const char* who = "d377_batch_fixed_msm_indexed_resident";
  if (t < 1 || t > (size_t)FX_MAX) return fail(D377_ERR_ARG, "%s: t must be 1 .. 64 terms per sum (D377_FIXED_BASES_MAX)", who);
  if (n && !base_index) return fail(D377_ERR_ARG, "%s: base_index is null", who);
  if (n && !scalar32) return fail(D377_ERR_ARG, "%s: scalar32 is null", who);
  if (n && !enc32_out) return fail(D377_ERR_ARG, "%s: enc32_out is null", who);
  if (!ctx) return fail(D377_ERR_ARG, "%s: ctx is null", who);
  std::lock_guard<std::mutex> lock(ctx->mu);
  ResidentCall c;
  const void* rec[3] = {scalar32, enc32_out, xyzt_out};
  int rc;
  if ((rc = resident_enter(who, ctx, dev, handle, rec, 3, base_index, verdict, &c))) return rc;
  if (n > SIZE_MAX / 32 / t) return fail(D377_ERR_ARG, "%s: n x t overflows", who);
  if (n == 0) return D377_OK;
  if (verdict && (rc = index_verdict_launch(*c.d, (hipStream_t)stream, base_index, n * t, (int)c.fb->m, verdict))) return rc;
  return fixed_msm_launch(*c.d, (hipStream_t)stream, *c.fb, c.tab, base_index, t, scalar32, n, enc32_out, xyzt_out);
}

// the verdict alone: for callers that want the host form's "nothing is computed" and read the record before they launch
int d377_check_base_index_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const int* base_index, size_t count,
                                   uint64_t* verdict) {
  const char* who = "d377_check_base_index_resident";
  if (count && !base_index) return fail(D377_ERR_ARG, "%s: base_index is null", who);
  if (!verdict) return fail(D377_ERR_ARG, "%s: verdict is null", who);
  if (!ctx) return fail(D377_ERR_ARG, "%s: ctx is null", who);
  std::lock_guard<std::mutex> lock(ctx->mu);
  ResidentCall c;
  int rc;
  if ((rc = resident_enter(who, ctx, dev, handle, nullptr, 0, base_index, verdict, &c))) return rc;
  return index_verdict_launch(*c.d, (hipStream_t)stream, base_index, count, (int)c.fb->m, verdict);
}

}  // extern "C"
