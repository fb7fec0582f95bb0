/*
 * decaf377_amd_ragged_sums.h -- many variable-base sums of ANY length each (0 .. 2^20 terms per sum), delimited by offsets, by
 * the bucket method: one call, the pipeline of d377_batch_bucket_msm (decaf377_amd_bucket_sums.h) with the sum of a term looked
 * up in the offsets.  Included at the end of decaf377_amd.h, which declares everything these prototypes use; include that
 * header.
 */
#ifndef DECAF377_AMD_RAGGED_SUMS_H
#define DECAF377_AMD_RAGGED_SUMS_H

#include "decaf377_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D377_BATCH_RAGGED_MSM_MAX_TERMS (1u << 20)   /* per sum */

/* n sums: enc32_out[i] = the Encoding of  sum over offsets[i] <= j < offsets[i + 1] of scalar32[j] * point[j].
 *   offsets        n + 1 values in HOST memory (also for the resident forms): offsets[0] == 0, the values never decrease, sum i
 *                  is the terms offsets[i] .. offsets[i + 1] - 1 of the term-major arrays and offsets[n] is the number of terms.
 *                  A length of 0 is allowed; a length above D377_BATCH_RAGGED_MSM_MAX_TERMS is refused.
 *   xyzt / enc32   offsets[n] Element records (128 bytes) or Encodings (32 bytes).  A record with Z = 0 counts as the identity.
 *                  An invalid Encoding is reported in status[j] (non-zero, offsets[n] bytes) and left out of its sum.
 *   scalar32       offsets[n] scalars, any 32 bytes, reduced mod r.
 *   enc32_out      n Encodings.  An empty sum gives what a sum of dead terms gives: the all-zero Encoding.
 *   xyzt_out       n Element records, or NULL; an empty sum's record is an identity record.
 *                  The records are reproducible byte for byte, like enc32_out and status: a call that returns records
 *                  orders the points of a bucket by their position in the input, as d377_batch_bucket_msm does.
 *   window_bits    0: the library's rule, d377_batch_bucket_msm's width for the MEAN length max(1, ceil(offsets[n] / n)).
 *                  4 .. 16 forces the width: a developer and test knob.  Whether the mean is the right statistic for skewed
 *                  lengths is an open item (see the sweep below).
 * How it runs.  Passes are greedy runs of consecutive sums: a pass of K sums takes the next one while (K + 1) 2^(window-1) <=
 * 2^17 and its points stay within 2^24.  Inside a pass everything is d377_batch_bucket_msm's, except that a term finds its sum
 * by a search over the pass's offsets (a workgroup of 256 terms first finds the sums of its first and last term).  A pass whose
 * sums are all empty runs no pipeline.  With equal lengths the passes, the width and the workspace are d377_batch_bucket_msm's
 * and so are the Encodings and statuses, byte for byte.
 * Arguments are checked in this order, the first four before any device is touched (all D377_ERR_ARG): n (n + 1 offsets must
 * not overflow), window_bits (the message names it), null offsets when n > 0, the offsets' values (offsets[0] != 0, a decrease
 * or a sum longer than the limit: the message names offsets and the index of the first offending sum), null xyzt / enc32,
 * scalar32, enc32_out, status (required only when offsets[n] > 0, except enc32_out: whenever n > 0), ctx; the resident forms
 * then dev, null offsets_dev and its 8-byte alignment, and the 16-byte alignment of the record buffers.  n == 0 with good
 * arguments is D377_OK.
 * The host forms upload the offsets themselves, slice the SUMS over the devices of a multi-GPU context -- each cut on the sum
 * boundary nearest to an equal share of TERMS --, copy in and out, bracket the kernels with the starvation check and
 * synchronise.
 * The resident forms take device pointers resident on device `dev` of the context, enqueue on `stream` and return.  They READ
 * THE HOST `offsets` BEFORE THEY RETURN (the checks, the pass cut and the workspace size come from it); the kernels read
 * `offsets_dev`, the same n + 1 values on the device, 8-byte aligned.  A RESIDENT CALL CANNOT VERIFY THAT THE TWO ARRAYS AGREE.
 * If they do not, the sums are wrong; memory stays safe, because the lookup clamps its result to the sums of the pass whatever
 * the array holds.  The rest is d377_batch_bucket_msm_resident's contract: no copy and no host synchronisation; the workspace
 * is exclusive per device and grows only outside a stream capture (D377_ERR_ARG inside one), so ONE EAGER CALL OF THE SHAPE
 * MUST COME FIRST; an outgrown workspace that a capture has seen is retired until d377_ctx_destroy, not freed; a replay must
 * not overlap another MSM of the same device on a different stream.  The output bytes are those of the host form.
 *
 * WHICH CALL WHERE.  This call has no short-sum route: every (window, sum) pair costs a workgroup of the tree of bit-sums and
 * every sum 2^(window-1) buckets of workspace, whatever its length.  When most sums are below about 1000 terms (the crossover
 * measured for equal lengths in decaf377_amd_bucket_sums.h), use d377_batch_segmented_msm (decaf377_amd_segmented_sums.h)
 * instead: the same arguments without window_bits, the same Encodings and statuses, by Straus chains;
 * d377_segmented_msm_plan's advised_route makes the choice.  One sum is d377_msm.  Equal lengths are d377_batch_bucket_msm (no offsets to keep in two
 * places).
 * Measured on one MI355X, device buffers, the legs alternating in one process, median of 5 after 2 warm-ups with each leg's
 * min-to-max spread, timed to the end of a device synchronise, the legs' Encodings compared
 * (profiles/ragged_sums_bench.json, tools/bench_ragged_sums.py):
 *   the cost of the lookup, equal lengths, this call / d377_batch_bucket_msm_resident on the same buffers --
 *     (n, m) = (2^8, 4096)  3.476 / 3.496 ms (spreads 0.064 / 0.042); (2^4, 2^16)  2.008 / 1.977 ms (spreads 0.107 / 0.117):
 *     the medians differ by less than the spreads at both shapes; the workspace is the uniform call's (1.60 GB and 0.79 GB).
 *   skewed lengths, 2^20 terms in 60 sums of 2^10 .. 2^16 terms (doubling, repeating), this call / the uniform call on every sum
 *   padded to 2^16 terms / one d377_msm_dev per sum --
 *     2.565 / 4.027 / 22.68 ms (spreads 0.088 / 0.101 / 0.101): USE THIS CALL, ahead of both by more than both spreads (x 1.6
 *     and x 8.8), in 0.88 GB of workspace against the padded call's 3.02 GB (d377_ragged_msm_plan / d377_bucket_msm_plan).
 *   window_bits swept on that skewed shape (profiles/ragged_sums_window_sweep.txt): 9 bits, the mean-length rule's width, 2.453
 *   ms (2.421 .. 2.493) and 10 bits 2.515 ms (2.455 .. 2.537) lie within each other's spread; 8 and 11 bits are behind (2.645,
 *   2.746 ms).  No width is ahead of the rule's on this shape; other skews have not been measured.
 */
int d377_batch_ragged_msm(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalar32, const uint64_t* offsets, size_t n,
                          int window_bits, uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_batch_ragged_msm_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, const uint64_t* offsets, size_t n,
                                  int window_bits, uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status);
int d377_batch_ragged_msm_resident(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalar32,
                                   const uint64_t* offsets, const uint64_t* offsets_dev, size_t n, int window_bits,
                                   uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_batch_ragged_msm_encoded_resident(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalar32,
                                           const uint64_t* offsets, const uint64_t* offsets_dev, size_t n, int window_bits,
                                           uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status);

/* The plan of such a call on device `dev`, without running it: the window width used (window_bits itself when forced), the
 * number of passes (0 when n == 0), the most sums and the most points a pass holds and the bytes of MSM workspace the call
 * needs (the largest pass's; 0 when no sum has a term).  Any out pointer may be NULL.  Checks n, window_bits and the offsets
 * as above, then ctx and dev. */
int d377_ragged_msm_plan(d377_ctx* ctx, int dev, const uint64_t* offsets, size_t n, int window_bits, int* window_bits_used,
                         uint64_t* passes, uint64_t* max_sums_per_pass, uint64_t* max_points_per_pass, uint64_t* workspace_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DECAF377_AMD_RAGGED_SUMS_H */
