// msm_ragged.inc -- d377_batch_ragged_msm (include/decaf377_amd_ragged_sums.h): many sums of ANY length each, delimited by
// offsets, through the pass of d377_batch_bucket_msm (msm_batch.inc: bsum_pass) with the term -> sum map taken from the offsets
// instead of i / m.  Included at the end of msm.hip, after msm_batch.inc.  The plan -- the lookup, the greedy pass cut, the
// width, the device slices -- is msm_ragged_plan.hpp's.
//
// A pass of K consecutive sums holding N points (the terms off[first] .. off[first + K] - 1 of the call, contiguous):
//   the prepare kernels, unchanged   over the pass's N points, scalars and statuses
//   k_rsum_keys       k_bsum_keys with the sum of term i looked up in the K + 1 offsets of the pass: a workgroup takes 256
//                     consecutive terms, finds the sums of its first and its last term (the same search in every lane, on
//                     addresses that depend on blockIdx alone) and each lane searches between the two
//   k_msm_count ... k_bsum_final     as in msm_batch.inc
// A pass without a point (all of its sums are empty) never enters the pipeline: k_rsum_empty writes what k_bsum_final writes
// for the identity.
#include "msm_ragged_plan.hpp"

namespace {

static_assert(RSUM_TILE == BLOCK, "k_rsum_keys: a workgroup is a tile");

// off: the K + 1 offsets of the pass, in terms of the call (off[0] = base is the pass's first term)
template <class DT>
__global__ void __launch_bounds__(BLOCK)
k_rsum_keys(const int16_t* digits, size_t n, const uint64_t* off, uint32_t K, uint64_t base, int W, int c, DT* keys) {
  for (size_t i0 = (size_t)blockIdx.x * BLOCK; i0 < n; i0 += (size_t)gridDim.x * BLOCK) {
    const size_t i1 = i0 + BLOCK - 1 < n ? i0 + BLOCK - 1 : n - 1;
    const uint32_t klo = rsum_sum_of_term(off, K, base + i0), khi = rsum_sum_of_term(off, K, base + i1);   // the tile's sums
    const size_t i = i0 + threadIdx.x;
    if (i >= n) continue;
    const uint32_t k = rsum_search(off, klo, khi, base + i);    // in 0 .. K - 1 whatever off holds
#pragma unroll 1
    for (int w = 0; w < W; ++w) keys[(size_t)w * n + i] = (DT)bsum_key(k, c, (int)digits[(size_t)w * n + i]);
  }
}

// the outputs of empty sum blockIdx.x: what k_bsum_final emits for the identity
__global__ void __launch_bounds__(64, 1)
k_rsum_empty(uint8_t* enc_out, uint64_t* xyzt_out) {
  const size_t k = blockIdx.x;
  msm_emit_doubled(ge_identity(), threadIdx.x == 0, enc_out + 32 * k, xyzt_out ? xyzt_out + 16 * k : nullptr);
}

// bsum_pass's map for a pass whose sums are delimited by offsets
struct RsumOffsets {
  const uint64_t* off_dev;                                       // the pass's K + 1 offsets on the device
  uint64_t base;                                                 // off[first]
  size_t n;                                                      // the points of the pass
  size_t points(size_t) const { return n; }
  template <class DT>
  void keys(DeviceState& d, hipStream_t s, const int16_t* dig, size_t N, size_t K, int W, int c, DT* out) const {
    hipLaunchKernelGGL(k_rsum_keys<DT>, dim3(grid_of(d, N)), dim3(BLOCK), 0, s, dig, N, off_dev, (uint32_t)K, base, W, c, out);
  }
};

// Everything on device pointers, enqueued on `s`; the caller holds ctx->mu and has selected the device.  off: the n + 1 offsets
// on the host (checked; off[0] need not be 0 here: a device's slice of a host call); off_dev: the same values on the device;
// the record buffers begin at term off[0].  c: the width of the call.
int rsum_launch(DeviceState& d, hipStream_t s, bool encoded, const void* pts_in, const uint8_t* scalars, const uint64_t* off,
                const uint64_t* off_dev, size_t n, int c, uint8_t* enc_out, uint64_t* xyzt_out, uint8_t* status) {
  if (n == 0) return D377_OK;
  int rc;
  if ((rc = msm_span_blocks(d))) return rc;
  const RsumPlan rp = rsum_plan(off, n, c, d.cus, d.msm_span_blocks);
  GuardScope held{d.msm_guard, s};
  if ((rc = msm_reserve(d, s, rp.bytes)) || (rc = held.acquire())) return rc;
  const size_t rec = encoded ? 32 : 128;
  for (size_t first = 0; first < n;) {
    const RsumPass ps = rsum_next_pass(off, n, first, c);
    uint8_t* eo = enc_out + first * 32;
    uint64_t* xo = xyzt_out ? xyzt_out + first * 16 : nullptr;
    if (ps.points == 0) {
      hipLaunchKernelGGL(k_rsum_empty, dim3((unsigned)ps.sums), dim3(64), 0, s, eo, xo);
      HIP_TRY(hipGetLastError());
    } else {
      const MsmPlan p = rsum_pass_plan(ps, c, d.cus, d.msm_span_blocks);
      const size_t t0 = (size_t)(off[first] - off[0]);
      const uint8_t* pts = (const uint8_t*)pts_in + t0 * rec;
      uint8_t* st = status ? status + t0 : nullptr;
      const RsumOffsets map{off_dev + first, off[first], ps.points};
      rc = p.wide_digits ? bsum_pass<int32_t>(d, s, p, encoded, pts, scalars + t0 * 32, map, ps.sums, eo, xo, st)
                         : bsum_pass<int16_t>(d, s, p, encoded, pts, scalars + t0 * 32, map, ps.sums, eo, xo, st);
      if (rc) return rc;
    }
    first += ps.sums;
  }
  return held.finish();
}

// What every form checks first, in the documented order and before any device is touched: n, window_bits, null offsets, the
// offsets' values, null buffers, ctx.  plan_only: d377_ragged_msm_plan, which has no buffers.
int rsum_check_args(d377_ctx* ctx, bool encoded, bool plan_only, const void* pts_in, const uint8_t* scalars, const uint64_t* off, size_t n,
                    int window_bits, const uint8_t* out32, const uint8_t* status) {
  if (n > (SIZE_MAX / 128) - 1) {
    snprintf(d377_g_err, sizeof d377_g_err, "batch_ragged_msm: n = %zu: n + 1 offsets and n records overflow", n);
    return D377_ERR_ARG;
  }
  if (window_bits != 0 && (window_bits < BSUM_MIN_WINDOW || window_bits > BSUM_MAX_WINDOW)) {
    snprintf(d377_g_err, sizeof d377_g_err, "batch_ragged_msm: window_bits = %d: 0 (the library's rule) or 4 .. 16", window_bits);
    return D377_ERR_ARG;
  }
  if (n) {
    if (!off) return fail(D377_ERR_ARG, "batch_ragged_msm: null buffer: %s", "offsets");
    if (off[0] != 0) {
      snprintf(d377_g_err, sizeof d377_g_err, "batch_ragged_msm: offsets [0] = %llu (sum 0): the first of the offsets must be 0",
               (unsigned long long)off[0]);
      return D377_ERR_ARG;
    }
    const size_t bad = rsum_first_bad_sum(off, n);
    if (bad < n) {
      if (off[bad + 1] < off[bad])
        snprintf(d377_g_err, sizeof d377_g_err, "batch_ragged_msm: offsets decrease at sum %zu: %llu after %llu", bad,
                 (unsigned long long)off[bad + 1], (unsigned long long)off[bad]);
      else
        snprintf(d377_g_err, sizeof d377_g_err,
                 "batch_ragged_msm: offsets give sum %zu %llu terms: at most 1048576 per sum (D377_BATCH_RAGGED_MSM_MAX_TERMS); d377_msm for "
                 "one longer sum", bad, (unsigned long long)(off[bad + 1] - off[bad]));
      return D377_ERR_ARG;
    }
    if (off[n] > SIZE_MAX / 128) return fail(D377_ERR_ARG, "%s", "batch_ragged_msm: offsets [n] x 128 overflows");
    if (!plan_only) {
      if (off[n]) {
        if (!pts_in) return fail(D377_ERR_ARG, "batch_ragged_msm: null buffer: %s", encoded ? "enc32" : "xyzt");
        if (!scalars) return fail(D377_ERR_ARG, "batch_ragged_msm: null buffer: %s", "scalar32");
      }
      if (!out32) return fail(D377_ERR_ARG, "batch_ragged_msm: null buffer: %s", "enc32_out");
      if (off[n] && encoded && !status) return fail(D377_ERR_ARG, "batch_ragged_msm: null buffer: %s", "status");
    }
  }
  if (!ctx) return fail(D377_ERR_ARG, "%s", "batch_ragged_msm: null context (ctx)");
  return D377_OK;
}

// one device's slice of a host batch: sums lo .. lo + n - 1 (off = offsets + lo); copies in, the passes, copies out, synchronised
int rsum_one(DeviceState& d, bool encoded, const uint8_t* pts_in, const uint8_t* scalars, const uint64_t* off, size_t n, int c, uint8_t* out32,
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
    if ((r = d.rsum_offsets.reserve(d.msm_guard, d.stream, (n + 1) * 8, SLACK_PARTIALS, "batch_ragged_msm: the offsets' area cannot grow inside a stream capture",
                                    "batch_ragged_msm: hipMalloc of the offsets' area failed (%zu bytes)")))
      return r;
    HIP_TRY(hipMemcpyAsync(d.rsum_offsets.mem, off, (n + 1) * 8, hipMemcpyHostToDevice, d.stream));
    if (terms) {
      HIP_TRY(hipMemcpyAsync(d.buf[0], pts_in, terms * rec, hipMemcpyHostToDevice, d.stream));
      HIP_TRY(hipMemcpyAsync(d.buf[1], scalars, terms * 32, hipMemcpyHostToDevice, d.stream));
    }
    if ((r = rsum_launch(d, d.stream, encoded, d.buf[0], d.buf[1], off, d.rsum_offsets.as<uint64_t>(), n, c, d.buf[2], xyzt_dev,
                         encoded ? d.buf[3] : nullptr)))
      return r;
    if ((r = sums_out_copy(d, n, out32, xyzt_out))) return r;
    if (encoded && terms) HIP_TRY(hipMemcpyAsync(status, d.buf[3], terms, hipMemcpyDeviceToHost, d.stream));
    return D377_OK;
  });
}

int rsum_host(d377_ctx* ctx, bool encoded, const void* pts_in, const uint8_t* scalars, const uint64_t* off, size_t n, int window_bits,
              uint8_t* out32, uint64_t* xyzt_out, uint8_t* status) {
  int rc;
  if ((rc = rsum_check_args(ctx, encoded, false, pts_in, scalars, off, n, window_bits, out32, status))) return rc;
  if (n == 0) return D377_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t rec = encoded ? 32 : 128, nd = ctx->devs.size();
  const int c = rsum_window(off[n], n, window_bits);             // one width for the call, whatever the slices hold
  // contiguous slices of the SUMS, cut where the TERMS are shared out evenly (rsum_device_cut): one unit per device
  return slice_over_devices(ctx, nd, [&](size_t k, size_t, size_t) {
    const size_t lo = rsum_device_cut(off, n, nd, k), hi = rsum_device_cut(off, n, nd, k + 1);
    const size_t t0 = (size_t)off[lo];
    return rsum_one(ctx->devs[k], encoded, (const uint8_t*)pts_in + t0 * rec, scalars + t0 * 32, off + lo, hi - lo, c, out32 + lo * 32,
                    xyzt_out ? xyzt_out + lo * 16 : nullptr, encoded ? status + t0 : nullptr);
  });
}

int rsum_resident(d377_ctx* ctx, int dev, void* stream, bool encoded, const void* pts_in, const uint8_t* scalars, const uint64_t* off,
                  const uint64_t* off_dev, size_t n, int window_bits, uint8_t* out32, uint64_t* xyzt_out, uint8_t* status) {
  int rc;
  if ((rc = rsum_check_args(ctx, encoded, false, pts_in, scalars, off, n, window_bits, out32, status))) return rc;
  if (dev < 0 || (size_t)dev >= ctx->devs.size()) return fail(D377_ERR_ARG, "%s", "batch_ragged_msm: dev is not a device of this context");
  if (n && !off_dev) return fail(D377_ERR_ARG, "batch_ragged_msm: null buffer: %s", "offsets_dev");
  if ((reinterpret_cast<uintptr_t>(off_dev) & 7u) != 0) return fail(D377_ERR_ARG, "%s", "batch_ragged_msm: offsets_dev must be 8-byte aligned");
  if (!aligned16(pts_in) || !aligned16(scalars) || !aligned16(out32) || !aligned16(xyzt_out))
    return fail(D377_ERR_ARG, "%s", "batch_ragged_msm: device record buffers must be 16-byte aligned");
  if (n == 0) return D377_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceState& d = ctx->devs[(size_t)dev];
  HIP_TRY(hipSetDevice(d.id));
  return rsum_launch(d, (hipStream_t)stream, encoded, pts_in, scalars, off, off_dev, n, rsum_window(off[n], n, window_bits), out32, xyzt_out,
                     status);
}

}  // namespace

extern "C" {

int d377_batch_ragged_msm(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalar32, const uint64_t* offsets, size_t n, int window_bits,
                          uint8_t* enc32_out, uint64_t* xyzt_out) {
  return rsum_host(ctx, false, xyzt, scalar32, offsets, n, window_bits, enc32_out, xyzt_out, nullptr);
}
int d377_batch_ragged_msm_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, const uint64_t* offsets, size_t n,
                                  int window_bits, uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status) {
  return rsum_host(ctx, true, enc32, scalar32, offsets, n, window_bits, enc32_out, xyzt_out, status);
}
int d377_batch_ragged_msm_resident(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalar32, const uint64_t* offsets,
                                   const uint64_t* offsets_dev, size_t n, int window_bits, uint8_t* enc32_out, uint64_t* xyzt_out) {
  return rsum_resident(ctx, dev, stream, false, xyzt, scalar32, offsets, offsets_dev, n, window_bits, enc32_out, xyzt_out, nullptr);
}
int d377_batch_ragged_msm_encoded_resident(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalar32,
                                           const uint64_t* offsets, const uint64_t* offsets_dev, size_t n, int window_bits, uint8_t* enc32_out,
                                           uint64_t* xyzt_out, uint8_t* status) {
  return rsum_resident(ctx, dev, stream, true, enc32, scalar32, offsets, offsets_dev, n, window_bits, enc32_out, xyzt_out, status);
}
int d377_ragged_msm_plan(d377_ctx* ctx, int dev, const uint64_t* offsets, size_t n, int window_bits, int* window_bits_used, uint64_t* passes,
                         uint64_t* max_sums_per_pass, uint64_t* max_points_per_pass, uint64_t* workspace_bytes) {
  int rc;
  if ((rc = rsum_check_args(ctx, false, true, nullptr, nullptr, offsets, n, window_bits, nullptr, nullptr))) return rc;
  if (dev < 0 || (size_t)dev >= ctx->devs.size()) return fail(D377_ERR_ARG, "%s", "batch_ragged_msm: dev is not a device of this context");
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceState& d = ctx->devs[(size_t)dev];
  HIP_TRY(hipSetDevice(d.id));
  if ((rc = msm_span_blocks(d))) return rc;
  const RsumPlan rp = rsum_plan(offsets, n, window_bits, d.cus, d.msm_span_blocks);
  if (window_bits_used) *window_bits_used = rp.c;
  if (passes) *passes = rp.passes;
  if (max_sums_per_pass) *max_sums_per_pass = rp.max_sums;
  if (max_points_per_pass) *max_points_per_pass = rp.max_points;
  if (workspace_bytes) *workspace_bytes = rp.bytes;
  return D377_OK;
}

}  // extern "C"
