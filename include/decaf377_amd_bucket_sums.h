/*
 * decaf377_amd_bucket_sums.h -- many variable-base sums of up to 2^20 terms each by the bucket method: one call, one run of
 * d377_msm's sort / span / bucket pipeline per pass for all the sums of the pass.  Included at the end of decaf377_amd.h,
 * which declares everything these prototypes use; include that header.
 */
#ifndef DECAF377_AMD_BUCKET_SUMS_H
#define DECAF377_AMD_BUCKET_SUMS_H

#include "decaf377_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D377_BATCH_BUCKET_MSM_MAX_TERMS (1u << 20)

/* n sums of m terms each: enc32_out[i] = the Encoding of  sum over j < m of scalar32[i m + j] * point[i m + j].
 * Semantics are d377_batch_msm_long[_encoded]'s:
 *   xyzt / enc32   n x m Element records (128 bytes) or Encodings (32 bytes), term-major: the m terms of sum 0, then of sum 1, ...
 *                  A record with Z = 0 counts as the identity.  An invalid Encoding is reported in status[i m + j] (non-zero)
 *                  and left out of its sum.
 *   scalar32       n x m scalars, any 32 bytes, reduced mod r.          1 <= m <= D377_BATCH_BUCKET_MSM_MAX_TERMS.
 *   enc32_out      n Encodings; a sum of nothing (every term dead or every scalar 0 mod r) gives the all-zero Encoding.
 *   xyzt_out       n Element records, or NULL.
 *   window_bits    0: the library's rule for the window width (a function of m).  4 .. 16 forces the width: A DEVELOPER AND
 *                  TEST KNOB (window sweeps, tests that need a given number of passes), not something to tune per call.
 * How it runs.  A pass holds K sums, K = min(n, 2^17 >> (window - 1), max(1, 2^24 / m)).  Every term's signed window digit d
 * (of k / 2 mod r, as in d377_msm) becomes the bucket key sign(d) * (s 2^(window-1) + |d|) for its sum s < K, so that one
 * counting sort, one generation of span sums and one per-bucket reduction serve all K sums; a tree of bit-sums per (window,
 * sum) and a Horner chain per sum finish.  The passes run back to back on the stream, in the device's MSM workspace sized for the
 * largest pass, with no host synchronisation in between.  Every m takes this route: there is no forwarding of short sums.
 * Arguments are checked in this order: m (D377_ERR_ARG; the message names m and points to d377_msm), window_bits
 * (D377_ERR_ARG; the message names window_bits) -- both before any device is touched --, null xyzt / enc32, scalar32,
 * enc32_out, status when n > 0, ctx; the resident forms then dev and the 16-byte alignment of the record buffers.  n == 0
 * with good arguments is D377_OK.
 * The host forms slice the SUMS over the devices of a multi-GPU context, copy in and out, bracket the kernels with the
 * starvation check and synchronise.
 * The resident forms take device pointers resident on device `dev` of the context (record buffers 16-byte aligned), enqueue on
 * `stream` (a hipStream_t, NULL = the default stream) and return: no copy, no host synchronisation, no allocation once the
 * workspace has grown to the shape; the context's mutex is held while enqueuing.  They obey d377_msm_dev's workspace rules: the
 * workspace is exclusive per device (calls on different streams queue behind each other); it grows only outside a stream
 * capture (D377_ERR_ARG inside one), so ONE EAGER CALL OF THE SHAPE MUST COME FIRST; once a captured launch has seen it, an
 * outgrown workspace is kept until d377_ctx_destroy instead of freed; a replay must not overlap another MSM of the same device
 * on a different stream.  The output bytes are those of the host form on the same inputs, status included.
 *
 * WHICH CALL WHERE.  Measured on one MI355X at 2^20 terms per call, device buffers, the legs alternating in one process, median
 * of 5 after 2 warm-ups with each leg's min-to-max spread, every leg timed to the end of a device synchronise and the legs'
 * Encodings compared (profiles/bucket_sums_bench.json, tools/bench_bucket_sums.py): this call's resident form /
 * d377_batch_long_msm_resident / n calls of d377_msm_dev on one stream --
 *   (n, m) = (2^12, 256)    18.09 / 7.35 / 990 ms (spreads 0.66 / 0.16 / 0.92): USE d377_batch_long_msm_resident INSTEAD, it is
 *                           ahead by more than both spreads; every (window, sum) pair costs this call a workgroup of the tree.
 *   (2^8, 4096)             3.65 / 7.43 / 91.4 ms (spreads 0.12 / 0.14 / 0.28): USE THIS CALL, ahead of both by more than both
 *                           spreads (x 2.0 and x 25).
 *   (2^4, 2^16)             1.95 / - / 7.29 ms (spreads 0.08 / 0.07): USE THIS CALL (x 3.7); the Straus forms stop at m = 4096.
 *   (1, 2^20)               1.597 / - / 1.588 ms (spreads 0.047 / 0.032): NOT ESTABLISHED, the medians differ by less than the
 *                           spreads; d377_msm is the call for one sum (no bookkeeping per sum, no window_bits to get wrong).
 * The crossover against d377_batch_long_msm_resident lies between m = 512 (10.20 against 7.31 ms) and m = 1024 (6.55 against
 * 7.04 ms, ahead by more than both spreads); m = 2048: 4.38 against 6.93 ms (profiles/bucket_sums_window_sweep.txt, which
 * also holds the sweep of window_bits that the width rule is fitted to).  Narrow windows over many sums cost memory: the
 * (2^12, 256) call reserves 6.5 GB of workspace, the (2^8, 4096) call 1.5 GB (d377_bucket_msm_plan reports it). */
int d377_batch_bucket_msm(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalar32, size_t m, size_t n, int window_bits,
                          uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_batch_bucket_msm_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, size_t m, size_t n, int window_bits,
                                  uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status);
int d377_batch_bucket_msm_resident(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalar32, size_t m,
                                   size_t n, int window_bits, uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_batch_bucket_msm_encoded_resident(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalar32,
                                           size_t m, size_t n, int window_bits, uint8_t* enc32_out, uint64_t* xyzt_out,
                                           uint8_t* status);

/* The plan of such a call on device `dev`, without running it: the window width used (window_bits itself when forced), the
 * sums per pass, the number of passes (0 when n == 0) and the bytes of MSM workspace the call needs.  Any out pointer may be
 * NULL.  Checks m and window_bits as above, then ctx and dev. */
int d377_bucket_msm_plan(d377_ctx* ctx, int dev, size_t n, size_t m, int window_bits, int* window_bits_used,
                         uint64_t* sums_per_pass, uint64_t* passes, uint64_t* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DECAF377_AMD_BUCKET_SUMS_H */
