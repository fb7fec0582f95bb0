/*
 * decaf377_amd_short_msm.h -- the one long sum (d377_msm) over scalars that are known to be short: 64 or 128 bits.
 * Included at the end of decaf377_amd.h, which declares everything these prototypes use; include that header.
 */
#ifndef DECAF377_AMD_SHORT_MSM_H
#define DECAF377_AMD_SHORT_MSM_H

#include "decaf377_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enc32_out = the Encoding of  sum over i < n of scalars[i] * point[i],  the scalars 8 or 16 bytes each.
 * The result is BYTE FOR BYTE what d377_msm[_encoded] returns for the same scalars zero-extended to 32 bytes.
 *   scalar_bytes   8 or 16.  Anything else is D377_ERR_ARG.
 *   scalars        n packed little-endian records of scalar_bytes bytes.  Every bit pattern is a scalar (2^128 < r): there
 *                  is no reduction, no validation pass and no status per scalar.
 *   xyzt / enc32   n Element records (128 bytes, read as they are; Z = 0 counts as the identity) or n Encodings (32 bytes;
 *                  an invalid one is reported in status[i], non-zero, and left out of the sum).
 *   enc32_out      one Encoding.  n == 0 gives what d377_msm gives: the all-zero Encoding of the identity.
 *   xyzt_out       one Element record, some representative of the sum, or NULL.
 *   n              below 2^31.
 * Why a call of its own.  d377_msm forms its sum with k / 2 mod r, which is a 251-bit number whatever k was, and cuts it into
 * ceil(252 / c) windows; the span sums, the sort and the Horner tail are proportional to the number of windows.  Here the
 * digits are those of k itself over the windows that tile 8 * scalar_bytes + 1 bits (the extra bit is the room the top window
 * needs for the carry of the signed digits below it): 5 windows for 64 bits and 9 for 128 where a full scalar takes 16 at 16-bit
 * windows, 6 and 11 against 21 at 12 bits.  The width is d377_msm's rule by n, then narrowed to the narrowest width that tiles
 * the bits with as many windows (65 bits asked for at 16: five windows of 13); d377_msm_short_plan reports what a call uses.
 * The sum is not a doubled half, so its Encoding takes a square root at the end of the call (d377_msm's takes an inversion);
 * its power chains run across the wave of the final kernel.  Every n takes the bucket route: the wave routes d377_msm has for
 * n up to a few thousand are not built for short scalars.
 *
 * WHICH CALL WHERE.  Measured on one MI355X, device buffers, Element records, this call against d377_msm_dev on the same values
 * zero-extended to 32 bytes, the legs alternating in one process, median of 5 after 2 warm-ups with each leg's min-to-max spread
 * (profiles/msm_short_bench.json, tools/bench_msm_short.py; a leg is ahead only where the medians differ by more than the two
 * spreads together), 8-byte / 16-byte scalars, ms:
 *   n = 256     0.367 / 0.409 against 0.267 / 0.268: USE d377_msm, its wave route is ahead by more than both spreads.
 *   n = 1024    0.355 against 0.388 (8 bytes): USE THIS CALL; 0.393 against 0.392 (16 bytes): NOT ESTABLISHED.
 *   n = 3072    0.348 / 0.397 against 0.498 / 0.513: USE THIS CALL.
 *   n = 2^12    0.368 / 0.402 against 0.724 / 0.589: USE THIS CALL (x 2.0 / x 1.5).
 *   n = 2^16    0.426 / 0.465 against 0.828 / 0.711: USE THIS CALL (x 1.9 / x 1.5).
 *   n = 2^20    0.787 / 1.139 against 2.073 / 2.615: USE THIS CALL (x 2.6 / x 2.3).
 *   n = 2^22    1.873 / 3.000 against 7.550 / 6.947: USE THIS CALL (x 4.0 / x 2.3).
 * Encodings as inputs and the host forms are not measured.
 * Arguments are checked in this order: scalar_bytes; null xyzt / enc32, scalars, enc32_out, status when n > 0, and n >= 2^31
 * -- all D377_ERR_ARG with the offender named, before any device is touched --; then ctx; the _dev forms then dev and the
 * alignment of the device buffers.
 * The host forms copy in and out (a quarter or half of d377_msm's scalar upload) and synchronise; a multi-GPU context sums
 * contiguous slices and combines the partial sums on its first device.
 * The _dev forms take device pointers resident on device `dev` of the context, enqueue on `stream` (a hipStream_t, NULL = the
 * default stream) and return.  Element records, Encodings and the outputs are 16-byte aligned as for d377_msm_dev; `scalars`
 * is aligned to scalar_bytes (D377_ERR_ARG otherwise).  They share d377_msm_dev's workspace and guard and obey its rules: the
 * workspace is exclusive per device (calls on different streams queue behind each other) and grows only outside a stream
 * capture, so ONE EAGER CALL OF THE SHAPE MUST COME FIRST. */
int d377_msm_short(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalars, int scalar_bytes, size_t n, uint8_t* enc32_out,
                   uint64_t* xyzt_out);
int d377_msm_short_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalars, int scalar_bytes, size_t n,
                           uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status);
int d377_msm_short_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalars, int scalar_bytes,
                       size_t n, uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_msm_short_encoded_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalars,
                               int scalar_bytes, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status);

/* The plan of such a call on device `dev`, without running it: the window width used (that of the wide windows; the rest are
 * one bit narrower), the number of windows and the bytes of MSM workspace the call needs.  Any out pointer may be NULL.  Checks
 * scalar_bytes and n as above, then ctx and dev. */
int d377_msm_short_plan(d377_ctx* ctx, int dev, size_t n, int scalar_bytes, int* window_bits_used, int* windows,
                        uint64_t* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DECAF377_AMD_SHORT_MSM_H */
