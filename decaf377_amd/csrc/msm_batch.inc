// msm_batch.inc -- d377_batch_bucket_msm (include/decaf377_amd_bucket_sums.h): many sums of up to 2^20 terms each through ONE
// run of the bucket method per pass, by the composite bucket key of msm_batch_plan.hpp.  Included at the end of msm.hip: it
// is a second caller of that unit's pipeline and lives in its translation unit.
//
// A pass of K sums of m terms (N = K m points):
//   the prepare kernels of msm.hip, unchanged   N points -> affine records; scalars -> the signed digits of c-bit windows (int16:
//                     c <= 16), staged in R_IDX, which nothing reads before the second placement level writes it
//   k_bsum_keys       digit d of point i, sum k = i / m  ->  key sign(d) (k 2^(c-1) + |d|) in R_DIGITS, int16 or int32 (one
//                     pass over the digits, 4-6 bytes per point and window, instead of a second copy of the three prepare kernels)
//   k_msm_count ... k_msm_buckets, unchanged    with nb' = K 2^(c-1) + 1 buckets per window: R_BUCKETS holds [W][nb'] records
//   k_bsum_block / k_bsum_block8   the block level of the tree of bit-sums over the 2^(c-1) leaves of pseudo-window (w, k):
//                     k_msm_wsum_block / _block8 with the leaves' base moved to w nb' + k 2^(c-1) + 1
//   k_msm_wsum_window, unchanged   one workgroup per pseudo-window: nodes and sums are [W K]
//   k_bsum_final      one wave per sum: k_msm_final's Horner chain over that sum's W window sums, the encoding
// The passes of a call run back to back on the stream in one workspace (the MSM workspace of the device, under its guard), with
// no host synchronisation in between; the Z != 1 flag and lvlmax are reset by every pass.
#include "msm_batch_plan.hpp"

namespace {

template <class DT>
__global__ void __launch_bounds__(BLOCK)
k_bsum_keys(const int16_t* digits, size_t n, size_t m, int W, int c, DT* keys) {
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * BLOCK) {
    const uint32_t k = (uint32_t)(i / m);
#pragma unroll 1
    for (int w = 0; w < W; ++w) keys[(size_t)w * n + i] = (DT)bsum_key(k, c, (int)digits[(size_t)w * n + i]);
  }
}

// leaf i of pseudo-window pw = w K + k: bucket record w nb + k 2^depth + 1 + i (the identity past the window's 2^depth leaves)
struct BsumLeaves {
  const uint32_t* first;
  int leaves;
  __device__ __forceinline__ BsumLeaves(const uint32_t* buckets, int pw, int nb, int depth, int K)
      : first(buckets + (bsum_leaf_base(pw / K, (size_t)(pw % K), nb, depth + 1) + 1) * PT_WORDS), leaves(1 << depth) {}
  __device__ __forceinline__ ge operator()(int i) const { return i < leaves ? pt_load_ext(first + (size_t)i * PT_WORDS) : ge_identity(); }
};

// k_msm_wsum_block (one wave, four leaves per lane, 2^m leaves per workgroup, 2 <= m <= WS_M) over pseudo-windows
__global__ void __launch_bounds__(WS_THREADS)
k_bsum_block(const uint32_t* buckets, int nb, int depth, int K, int m, int nblk, uint32_t* nodes) {
  __shared__ uint32_t lds[(WSA_CAP0 + WSA_CAP1) * LP_WORDS];
  const int pw = blockIdx.x / nblk, blk = blockIdx.x % nblk, t = threadIdx.x;
  LdsPts A{lds, WSA_CAP0}, B{lds + WSA_CAP0 * LP_WORDS, WSA_CAP1};
  const BsumLeaves leaf(buckets, pw, nb, depth, K);
  const int M1 = 1 << (m - 2);                                 // nodes after level 1
  if (t < M1) {                                                // leaves 4t .. 4t + 3: T = B0 + B1 + B2 + B3, V_0 = B1 + B3, V_1 = B2 + B3
    const int l0 = (blk << m) + 4 * t;
    const ge p0 = leaf(l0), p1 = leaf(l0 + 1), p2 = leaf(l0 + 2), p3 = leaf(l0 + 3);
    const ge r = ge_add(p2, p3);
    A.store(3 * t, ge_add(ge_add(p0, p1), r));
    A.store(3 * t + 1, ge_add(p1, p3));
    A.store(3 * t + 2, r);
  }
  __syncthreads();
  LdsPts cur = A, nxt = B;
#pragma unroll 1
  for (int j = 2; j < m; ++j) {
    wsum_level_any(cur, nxt, j, M1 >> (j - 1), t, WS_THREADS);
    __syncthreads();
    const LdsPts tmp = cur; cur = nxt; nxt = tmp;
  }
  if (t <= m) pt_store_ext(nodes + (((size_t)pw * nblk + blk) * NODE_STRIDE + t) * PT_WORDS, cur.load(t));
}

// k_msm_wsum_block8 (eight leaves per lane, 512 per one-wave workgroup, the levels in place; m == WS_M8) over pseudo-windows
__global__ void __launch_bounds__(WS8_THREADS)
k_bsum_block8(const uint32_t* buckets, int nb, int depth, int K, int m, int nblk, uint32_t* nodes) {
  __shared__ uint32_t lds[WS8_CAP * LP_WORDS];
  const int pw = blockIdx.x / nblk, blk = blockIdx.x % nblk, t = threadIdx.x;
  LdsPts A{lds, WS8_CAP};
  {
    const BsumLeaves at(buckets, pw, nb, depth, K);
    const int l0 = (blk << m) + 8 * t;
    auto leaf = [&](int i) { return at(l0 + i); };
    // T = sum of the eight, V_0 = odd leaves, V_1 = leaves 2 3 6 7, V_2 = leaves 4..7: 11 additions, leaves streamed
    ge s, a23;
    const ge p1 = leaf(1), p3 = leaf(3);
    const ge o13 = ge_add(p1, p3);
    const ge a01 = ge_add(leaf(0), p1);
    a23 = ge_add(leaf(2), p3);
    s = ge_add(a01, a23);
    const ge p5 = leaf(5), p7 = leaf(7);
    A.store(4 * t + 1, ge_add(o13, ge_add(p5, p7)));
    const ge a45 = ge_add(leaf(4), p5), a67 = ge_add(leaf(6), p7);
    A.store(4 * t + 2, ge_add(a23, a67));
    const ge v2 = ge_add(a45, a67);
    A.store(4 * t + 3, v2);
    A.store(4 * t, ge_add(s, v2));
  }
  __syncthreads();
#pragma unroll 1
  for (int j = 3; j < m; ++j) wsum_level_inplace(A, j, WS8_THREADS >> (j - 2), t);
  if (t <= m) pt_store_ext(nodes + (((size_t)pw * nblk + blk) * NODE_STRIDE + t) * PT_WORDS, A.load(t));
}

// k_msm_final for sum k = blockIdx.x: Horner over the window sums S_(w, k) = sums[w K + k] in the lane-spread form, the
// doubling that undoes the halved scalars, the encoding and (optional) the Element record of sum k
__global__ void __launch_bounds__(64, 1)
k_bsum_final(const uint32_t* sums, WinShape ws, int K, uint8_t* enc_out, uint64_t* xyzt_out) {
  const int W = ws.W, k = blockIdx.x;
  __shared__ uint32_t crec[63 * RQ_WORDS];
  const int t = threadIdx.x;
  if (t < W - 1) rq_store_cached(crec + t * RQ_WORDS, pt_load_ext(sums + ((size_t)t * K + k) * PT_WORDS));
  if (t == W - 1) rq_store_point(crec + (W - 1) * RQ_WORDS, pt_load_ext(sums + ((size_t)(W - 1) * K + k) * PT_WORDS));
  __syncthreads();
  const row::RowK RK = row::row_consts();
  const row::RowSel S = row::row_sel();
  uint32_t v = crec[(W - 1) * RQ_WORDS + t];
  bool negated = false;                                          // v holds minus the running sum
#pragma unroll 1
  for (int w = W - 2; w >= 0; --w) {
    const int c = ws.width(w);
#pragma unroll 1
    for (int j = 0; j < c; ++j) v = row::rq_double_neg(v, S, RK);
    if (c & 1) negated = !negated;
    v = row::rq_add(v, crec + w * RQ_WORDS, S, negated, RK);
  }
  __syncthreads();
  crec[t] = v;
  __syncthreads();
  ge r = rq_load_point(crec);
  if (negated) r = ge_neg(r);
  msm_emit_doubled(r, t == 0, enc_out + (size_t)32 * k, xyzt_out ? xyzt_out + (size_t)16 * k : nullptr);
}

// ------------------------------------------------------------------------------ host side ---
// Which term belongs to which sum, the one thing a pass needs to know about the lengths: the points of a pass of K sums and
// the launch of its keys kernel.  Equal lengths here; offsets in msm_ragged.inc (RsumOffsets).
struct BsumEqual {
  size_t m;
  size_t points(size_t K) const { return K * m; }
  template <class DT>
  void keys(DeviceState& d, hipStream_t s, const int16_t* dig, size_t N, size_t, int W, int c, DT* out) const {
    hipLaunchKernelGGL(k_bsum_keys<DT>, dim3(grid_of(d, N)), dim3(BLOCK), 0, s, dig, N, m, W, c, out);
  }
};

// one pass: K sums, their terms dealt by `map`, under plan p (msm_plan with sums = K), in the workspace the caller holds
template <class DT, class Map>
int bsum_pass(DeviceState& d, hipStream_t s, const MsmPlan& p, bool encoded, const void* pts_in, const uint8_t* scalars, const Map& map, size_t K,
              uint8_t* enc_out, uint64_t* xyzt_out, uint8_t* status) {
  const size_t N = map.points(K);
  const MsmCall call{d, s, p, N, xyzt_out != nullptr};         // records are returned: their bytes are a function of the inputs
  int rc;
  int16_t* dig = msm_at<int16_t>(call, R_IDX);                  // the plain digits: W N int16 in a region of W N words
  if ((rc = msm_prepare<int16_t>(call, encoded, pts_in, scalars, status, dig))) return rc;
  map.template keys<DT>(d, s, dig, N, K, p.W, p.shape.c, msm_at<DT>(call, R_DIGITS));
  if ((rc = msm_count<DT>(call))) return rc;
  if ((rc = msm_scan_place(call))) return rc;
  if ((rc = msm_bucket_records(call))) return rc;
  uint32_t *bkt = msm_at(call, R_BUCKETS), *nodes = msm_at(call, R_NODES), *sums = msm_at(call, R_SUMS);
  const dim3 blocks((unsigned)(p.pw * p.ws_nblk));
  if (p.block_kernel == WSUM_BLOCK8) hipLaunchKernelGGL(k_bsum_block8, blocks, dim3(WS8_THREADS), 0, s, bkt, p.nb, p.ws_depth, (int)K, p.ws_m, p.ws_nblk, nodes);
  else hipLaunchKernelGGL(k_bsum_block, blocks, dim3(WS_THREADS), 0, s, bkt, p.nb, p.ws_depth, (int)K, p.ws_m, p.ws_nblk, nodes);
  if (p.wsb_lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_msm_wsum_window), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.wsb_lds));
  hipLaunchKernelGGL(k_msm_wsum_window, dim3((unsigned)p.pw), dim3(WSB_THREADS), p.wsb_lds, s, nodes, p.ws_depth, p.top_m, p.top_nblk, p.top_stride, p.cap0,
                     p.cap1, sums);
  hipLaunchKernelGGL(k_bsum_final, dim3((unsigned)K), dim3(64), 0, s, sums, p.shape, (int)K, enc_out, xyzt_out);
  HIP_TRY(hipGetLastError());
  return D377_OK;
}

BsumPlan bsum_plan_for(DeviceState& d, size_t n, size_t m, int window_bits) {
  return bsum_plan(BsumPlanIn{n, m, window_bits, d.cus, d.msm_span_blocks});
}

// everything on device pointers, enqueued on `s`; the caller holds ctx->mu and has selected the device
int bsum_launch(DeviceState& d, hipStream_t s, bool encoded, const void* pts_in, const uint8_t* scalars, size_t m, size_t n, int window_bits,
                uint8_t* enc_out, uint64_t* xyzt_out, uint8_t* status) {
  if (n == 0) return D377_OK;
  int rc;
  if ((rc = msm_span_blocks(d))) return rc;
  const BsumPlan bp = bsum_plan_for(d, n, m, window_bits);
  GuardScope held{d.msm_guard, s};
  if ((rc = msm_reserve(d, s, bp.bytes)) || (rc = held.acquire())) return rc;
  const size_t rec = encoded ? 32 : 128;
  for (size_t pass = 0; pass < bp.passes; ++pass) {
    const size_t lo = pass * bp.sums_per_pass, K = pass + 1 < bp.passes ? bp.sums_per_pass : bp.last_sums;
    const MsmPlan& p = pass + 1 < bp.passes ? bp.full : bp.last;
    const uint8_t* pts = (const uint8_t*)pts_in + lo * m * rec;
    uint64_t* xo = xyzt_out ? xyzt_out + lo * 16 : nullptr;
    uint8_t* st = status ? status + lo * m : nullptr;
    rc = p.wide_digits ? bsum_pass<int32_t>(d, s, p, encoded, pts, scalars + lo * m * 32, BsumEqual{m}, K, enc_out + lo * 32, xo, st)
                       : bsum_pass<int16_t>(d, s, p, encoded, pts, scalars + lo * m * 32, BsumEqual{m}, K, enc_out + lo * 32, xo, st);
    if (rc) return rc;
  }
  return held.finish();
}

// What every form checks first, in the documented order and before any device is touched: m, window_bits, null buffers
// (n > 0), ctx.
int bsum_check_args(d377_ctx* ctx, bool encoded, const void* pts_in, const uint8_t* scalars, size_t m, size_t n, int window_bits,
                    const uint8_t* out32, const uint8_t* status) {
  if (m < 1 || m > BSUM_MAX_TERMS) {
    snprintf(d377_g_err, sizeof d377_g_err,
             "batch_bucket_msm: m = %zu: 1 .. 1048576 terms per sum (D377_BATCH_BUCKET_MSM_MAX_TERMS); d377_msm for one longer sum", m);
    return D377_ERR_ARG;
  }
  if (window_bits != 0 && (window_bits < BSUM_MIN_WINDOW || window_bits > BSUM_MAX_WINDOW)) {
    snprintf(d377_g_err, sizeof d377_g_err, "batch_bucket_msm: window_bits = %d: 0 (the library's rule) or 4 .. 16", window_bits);
    return D377_ERR_ARG;
  }
  if (n) {
    if (!pts_in) return fail(D377_ERR_ARG, "batch_bucket_msm: null buffer: %s", encoded ? "enc32" : "xyzt");
    if (!scalars) return fail(D377_ERR_ARG, "batch_bucket_msm: null buffer: %s", "scalar32");
    if (!out32) return fail(D377_ERR_ARG, "batch_bucket_msm: null buffer: %s", "enc32_out");
    if (encoded && !status) return fail(D377_ERR_ARG, "batch_bucket_msm: null buffer: %s", "status");
  }
  if (!ctx) return fail(D377_ERR_ARG, "%s", "batch_bucket_msm: null context (ctx)");
  if (n > SIZE_MAX / 128 / m) return fail(D377_ERR_ARG, "%s", "batch_bucket_msm: n x m overflows");
  return D377_OK;
}

// one device's slice of a host batch: copies in, the passes, copies out, synchronised
int bsum_one(DeviceState& d, bool encoded, const uint8_t* pts_in, const uint8_t* scalars, size_t m, size_t n, int window_bits, uint8_t* out32,
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
    if ((r = bsum_launch(d, d.stream, encoded, d.buf[0], d.buf[1], m, n, window_bits, d.buf[2], xyzt_dev, encoded ? d.buf[3] : nullptr))) return r;
    if ((r = sums_out_copy(d, n, out32, xyzt_out))) return r;
    if (encoded) HIP_TRY(hipMemcpyAsync(status, d.buf[3], terms, hipMemcpyDeviceToHost, d.stream));
    return D377_OK;
  });
}

int bsum_host(d377_ctx* ctx, bool encoded, const void* pts_in, const uint8_t* scalars, size_t m, size_t n, int window_bits, uint8_t* out32,
              uint64_t* xyzt_out, uint8_t* status) {
  int rc;
  if ((rc = bsum_check_args(ctx, encoded, pts_in, scalars, m, n, window_bits, out32, status))) return rc;
  if (n == 0) return D377_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  const size_t rec = encoded ? 32 : 128;
  // contiguous slices of the SUMS over the context's devices (host_state.hpp: slice_over_devices)
  return slice_over_devices(ctx, n, [&](size_t k, size_t lo, size_t cnt) {
    return bsum_one(ctx->devs[k], encoded, (const uint8_t*)pts_in + lo * m * rec, scalars + lo * m * 32, m, cnt, window_bits, out32 + lo * 32,
                    xyzt_out ? xyzt_out + lo * 16 : nullptr, encoded ? status + lo * m : nullptr);
  });
}

int bsum_resident(d377_ctx* ctx, int dev, void* stream, bool encoded, const void* pts_in, const uint8_t* scalars, size_t m, size_t n,
                  int window_bits, uint8_t* out32, uint64_t* xyzt_out, uint8_t* status) {
  int rc;
  if ((rc = bsum_check_args(ctx, encoded, pts_in, scalars, m, n, window_bits, out32, status))) return rc;
  if (dev < 0 || (size_t)dev >= ctx->devs.size()) return fail(D377_ERR_ARG, "%s", "batch_bucket_msm: dev is not a device of this context");
  if (!aligned16(pts_in) || !aligned16(scalars) || !aligned16(out32) || !aligned16(xyzt_out))
    return fail(D377_ERR_ARG, "%s", "batch_bucket_msm: device record buffers must be 16-byte aligned");
  if (n == 0) return D377_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceState& d = ctx->devs[(size_t)dev];
  HIP_TRY(hipSetDevice(d.id));
  return bsum_launch(d, (hipStream_t)stream, encoded, pts_in, scalars, m, n, window_bits, out32, xyzt_out, status);
}

}  // namespace

extern "C" {

int d377_batch_bucket_msm(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalar32, size_t m, size_t n, int window_bits,
                          uint8_t* enc32_out, uint64_t* xyzt_out) {
  return bsum_host(ctx, false, xyzt, scalar32, m, n, window_bits, enc32_out, xyzt_out, nullptr);
}
int d377_batch_bucket_msm_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, size_t m, size_t n, int window_bits,
                                  uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status) {
  return bsum_host(ctx, true, enc32, scalar32, m, n, window_bits, enc32_out, xyzt_out, status);
}
int d377_batch_bucket_msm_resident(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalar32, size_t m, size_t n,
                                   int window_bits, uint8_t* enc32_out, uint64_t* xyzt_out) {
  return bsum_resident(ctx, dev, stream, false, xyzt, scalar32, m, n, window_bits, enc32_out, xyzt_out, nullptr);
}
int d377_batch_bucket_msm_encoded_resident(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalar32, size_t m,
                                           size_t n, int window_bits, uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status) {
  return bsum_resident(ctx, dev, stream, true, enc32, scalar32, m, n, window_bits, enc32_out, xyzt_out, status);
}
int d377_bucket_msm_plan(d377_ctx* ctx, int dev, size_t n, size_t m, int window_bits, int* window_bits_used, uint64_t* sums_per_pass,
                         uint64_t* passes, uint64_t* workspace_bytes) {
  static const uint8_t some = 0;                                  // (the buffers are not this call's business)
  int rc;
  if ((rc = bsum_check_args(ctx, false, &some, &some, m, 0, window_bits, &some, nullptr))) return rc;
  if (dev < 0 || (size_t)dev >= ctx->devs.size()) return fail(D377_ERR_ARG, "%s", "batch_bucket_msm: dev is not a device of this context");
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceState& d = ctx->devs[(size_t)dev];
  HIP_TRY(hipSetDevice(d.id));
  if ((rc = msm_span_blocks(d))) return rc;
  const BsumPlan bp = bsum_plan_for(d, n, m, window_bits);
  if (window_bits_used) *window_bits_used = bp.c;
  if (sums_per_pass) *sums_per_pass = bp.sums_per_pass;
  if (passes) *passes = n ? bp.passes : 0;
  if (workspace_bytes) *workspace_bytes = bp.bytes;
  return D377_OK;
}

}  // extern "C"
