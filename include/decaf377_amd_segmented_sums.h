/*
 * decaf377_amd_segmented_sums.h -- many variable-base sums of ANY length each (0 .. 2^20 terms per sum), delimited by offsets,
 * by Straus chains: the counterpart of d377_batch_msm_long (decaf377_amd_long_sums.h) for sums of unequal length, and the
 * short-sum route that d377_batch_ragged_msm (decaf377_amd_ragged_sums.h, the bucket pipeline) does not have.  Included at the
 * end of decaf377_amd.h, which declares everything these prototypes use; include that header.
 */
#ifndef DECAF377_AMD_SEGMENTED_SUMS_H
#define DECAF377_AMD_SEGMENTED_SUMS_H

#include "decaf377_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define D377_BATCH_SEGMENTED_MSM_MAX_TERMS (1u << 20)   /* per sum: D377_BATCH_RAGGED_MSM_MAX_TERMS */
#define D377_SEGMENTED_ROUTE_CHAINS 0                    /* advised_route of d377_segmented_msm_plan */
#define D377_SEGMENTED_ROUTE_BUCKETS 1

/* n sums: enc32_out[i] = the Encoding of  sum over offsets[i] <= j < offsets[i + 1] of scalar32[j] * point[j].
 * The arguments are d377_batch_ragged_msm's, without window_bits:
 *   offsets        n + 1 values in HOST memory (also for the resident forms): offsets[0] == 0, the values never decrease, sum i
 *                  is the terms offsets[i] .. offsets[i + 1] - 1 of the term-major arrays and offsets[n] is the number of terms.
 *                  A length of 0 is allowed; a length above D377_BATCH_SEGMENTED_MSM_MAX_TERMS is refused.  Every input that
 *                  d377_batch_ragged_msm accepts is accepted here.
 *   xyzt / enc32   offsets[n] Element records (128 bytes) or Encodings (32 bytes).  A record with Z = 0 counts as the identity.
 *                  An invalid Encoding is reported in status[j] (non-zero, offsets[n] bytes) and left out of its sum.
 *   scalar32       offsets[n] scalars, any 32 bytes, reduced mod r.
 *   enc32_out      n Encodings.  An empty sum gives the all-zero Encoding.
 *   xyzt_out       n Element records, or NULL; an empty sum's record is an identity record.  The records are SOME
 *                  representative of the group element: not d377_batch_ragged_msm's bytes.
 * The Encodings and statuses are d377_batch_ragged_msm's byte for byte, and with equal lengths of up to 4096 d377_batch_msm_long's.
 * How it runs.  Sum i of length L is cut as d377_batch_msm_long cuts it: g = ceil(L / 8) chains of b = ceil(L / g) terms.  No
 * table is built on the host: the chains of sum i lie from slot floor(offsets[i] / 8) + i of a space of floor(T / 8) + n
 * records (T = offsets[n]; at most n of them unused), and the lane -- or, up to four slots per SIMD, the wave -- of a slot
 * finds its sum by a binary search over that expression.  The fold places its levels by the same step (16 records per
 * lane); a last level adds the at most 16 records a sum has left, and the chunked compressor writes the n Encodings.
 * KNOWN COST, UNMEASURED: the lanes of a wave run chains of 1 .. 8 terms side by side, so a wave takes as long as its longest
 * chain, and sums below 8 terms leave table scratch unused.  Chains are neither sorted nor binned by length.
 * Arguments are checked in this order, the first three before any device is touched (all D377_ERR_ARG): n (n + 1 offsets must
 * not overflow), null offsets when n > 0, the offsets' values (offsets[0] != 0, a decrease or a sum longer than the limit: the
 * message names offsets and the index of the first offending sum), null xyzt / enc32, scalar32, enc32_out, status (required
 * only when offsets[n] > 0, except enc32_out: whenever n > 0), ctx; the resident forms then dev, null offsets_dev and its
 * 8-byte alignment, and the 16-byte alignment of the record buffers.  n == 0 with good arguments is D377_OK.
 * The host forms upload the offsets themselves, slice the SUMS over the devices of a multi-GPU context at
 * d377_batch_ragged_msm's cuts -- the sum boundary nearest to an equal share of TERMS --, copy in and out, bracket the kernels
 * with the starvation check and synchronise.
 * The resident forms take device pointers resident on device `dev` of the context, enqueue on `stream` and return.  They READ
 * THE HOST `offsets` BEFORE THEY RETURN (the checks, the number of fold levels and the scratch size come from it); the kernels
 * read `offsets_dev`, the same n + 1 values on the device, 8-byte aligned.  A RESIDENT CALL CANNOT VERIFY THAT THE TWO ARRAYS
 * AGREE.  If they do not, the sums are wrong; memory stays safe: every lookup clamps to the sums 0 .. n - 1, no term from
 * offsets[n] on is read and every record index stays inside the area sized from the host array.  No copy, no host
 * synchronisation and, once the scratch has grown, no allocation.  The scratch (the long sums' partials area and table
 * scratch) grows only outside a stream capture (D377_ERR_ARG inside one), so ONE EAGER CALL OF THE SHAPE MUST COME FIRST; an
 * outgrown area that a capture has seen is retired until d377_ctx_destroy, not freed.  The output bytes are those of the host form.
 *
 * WHICH CALL WHERE.  d377_segmented_msm_plan's advised_route: this call while the mean length of the non-empty sums is below
 * 1024 terms, d377_batch_ragged_msm from there on.  Equal lengths of up to 4096 are d377_batch_msm_long.
 * Measured on one MI355X at 2^20 terms per call, device buffers, the legs alternating in one process, median of 5 after 2
 * warm-ups with each leg's min-to-max spread, timed to the end of a device synchronise, the legs' Encodings compared; a leg is
 * ahead only where the medians differ by more than the two spreads together (profiles/segmented_sums_bench.json,
 * tools/bench_segmented_sums.py):
 *   the cost of the lookup and of the slot space, equal lengths, this call / d377_batch_long_msm_resident on the same buffers --
 *     (n, m) = (2^16, 16)  8.791 / 6.422 ms (spreads 0.137 / 0.149); (2^12, 256)  9.007 / 6.959 ms (spreads 0.045 / 0.128): USE
 *     THE OTHER at both shapes; the scratch is 1.88 GB and 1.86 GB (d377_segmented_msm_plan).  At 2^20 terms the long sums have
 *     exactly one chain per resident lane, and this call's dead slots push its lane kernel into a second round: the supposed
 *     cause, not separated by a measurement.
 *   skewed short sums, 2^20 terms in 2825 sums of 2 .. 2048 terms (doubling, repeating; mean 372), this call /
 *   d377_batch_ragged_msm_resident on the same buffers / d377_batch_long_msm_indexed_resident padded to 2048 terms with -1 --
 *     9.527 / 13.00 / 31.48 ms (spreads 0.080 / 0.178 / 0.421): USE THIS CALL, ahead of both (x 1.4 and x 3.3), in 1.86 GB of
 *     scratch against the ragged call's 4.98 GB of workspace.
 *   the crossover behind advised_route, equal lengths, d377_batch_long_msm_resident / d377_batch_bucket_msm_resident --
 *     512: 7.261 / 10.312 ms, 640: 7.290 / 8.774, 768: 7.206 / 7.809, 896: 7.181 / 7.120 (spreads 0.160 / 0.064: not
 *     established), 1024: 7.088 / 6.595 (spreads 0.132 / 0.137).  The smallest length with the buckets ahead is 1024:
 *     ESTABLISHED BY THIS SWEEP, and equal to the point measured before.
 */
int d377_batch_segmented_msm(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalar32, const uint64_t* offsets, size_t n,
                             uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_batch_segmented_msm_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, const uint64_t* offsets, size_t n,
                                     uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status);
int d377_batch_segmented_msm_resident(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalar32,
                                      const uint64_t* offsets, const uint64_t* offsets_dev, size_t n, uint8_t* enc32_out,
                                      uint64_t* xyzt_out);
int d377_batch_segmented_msm_encoded_resident(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalar32,
                                              const uint64_t* offsets, const uint64_t* offsets_dev, size_t n, uint8_t* enc32_out,
                                              uint64_t* xyzt_out, uint8_t* status);

/* The plan of such a call on device `dev`, without running it: the slots of the chains' space (floor(T / 8) + n), the chains
 * that run (the others are dead), the slot-indexed fold levels, the most terms a chain holds (0 when no sum has a term), the
 * bytes of scratch the call needs (the partials area and, above four slots per SIMD, the lanes' table scratch) and the
 * advised route (D377_SEGMENTED_ROUTE_*).  Any out pointer may be NULL.  Checks n and the offsets as above, then ctx and dev. */
int d377_segmented_msm_plan(d377_ctx* ctx, int dev, const uint64_t* offsets, size_t n, uint64_t* chain_slots, uint64_t* chains,
                            int* fold_levels, int* max_slots_per_chain, uint64_t* scratch_bytes, int* advised_route);

#ifdef __cplusplus
}
#endif
#endif /* DECAF377_AMD_SEGMENTED_SUMS_H */
