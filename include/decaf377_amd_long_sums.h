/*
 * decaf377_amd_long_sums.h -- the long variable-base sums (d377_batch_msm_long) on device buffers, and long sums whose terms
 * name their points in a shared pool.  Included at the end of decaf377_amd.h, which declares everything these prototypes
 * use; include that header.  The names read `long_msm`, as d377_batch_fixed_long_msm does: the library keeps `msm_long` in
 * its exports for the two host forms of decaf377_amd.h alone (tests/test_batch_msm_long_host.py).
 */
#ifndef DECAF377_AMD_LONG_SUMS_H
#define DECAF377_AMD_LONG_SUMS_H

#include "decaf377_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The resident forms of d377_batch_msm_long[_encoded]: the host form's arguments behind `int dev, void* stream`, under the
 * contract decaf377_amd_resident.h states for its family.  Every pointer is a device pointer resident on device `dev` of the
 * context; the record buffers (points or Encodings, scalars, enc32_out, xyzt_out) are 16-byte aligned, anything else is
 * D377_ERR_ARG; the call enqueues on `stream` (a hipStream_t, NULL = the default stream) and returns, with no copy, no host
 * synchronisation and no allocation once the scratch areas have grown to the shape; the context's mutex is held while
 * enqueuing; starvation is the caller's check (d377_ctx_starved_counter_dev / d377_ctx_health).  Arguments are checked in the
 * host form's order with its texts -- m, null buffers when n > 0, ctx -- then dev and the alignment; n == 0 with good
 * arguments is D377_OK and enqueues nothing.  The output bytes are those of the host form on the same inputs, status
 * included.  For m <= 8 the calls forward to d377_batch_msm_small[_encoded]_dev; longer sums run the host form's launch on
 * the caller's buffers.
 * Graphs: as decaf377_amd_resident.h says of its calls.  The table scratch and the partial sums' area cannot grow inside a
 * stream capture (D377_ERR_ARG), so ONE EAGER CALL OF THE SHAPE MUST COME FIRST; an area that a captured launch has seen is
 * kept until d377_ctx_destroy when a later call outgrows it; a replay must not overlap another batched-sum call of the same
 * device on a different stream. */
int d377_batch_long_msm_resident(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalar32, size_t m,
                                 size_t n, uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_batch_long_msm_encoded_resident(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalar32,
                                         size_t m, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status);

/* Long sums whose terms NAME their points: sum i = sum over j < m of scalar32[i m + j] * pool[point_index[i m + j]].
 * d377_batch_msm_long carries a 128-byte record per term; sums that draw on a common set of points -- vector commitments
 * over the same ad-hoc generators, verification equations that reuse keys, sums over subsets of one commitment list -- name
 * the point instead: 36 bytes per term.  (Points worth registering have the fixed-base combs; a pool costs nothing to
 * build and may change from call to call.)
 *   pool_xyzt     pool_count Element records, 1 <= pool_count <= 2^31 - 1 (Elements only: a caller with Encodings
 *                 decompresses the pool once).  A record with Z = 0 counts as the identity.
 *   point_index   n x m ints.  An index may repeat within a sum and across sums.  -1 is an ABSENT term: it reads no point and
 *                 no scalar, contributes nothing and costs a slot -- so m is the longest sum's length and shorter sums end in
 *                 -1.  A sum whose terms are all absent gives the all-zero Encoding.
 *   scalar32      n x m scalars, any 32 bytes, reduced mod r.     1 <= m <= D377_BATCH_MSM_LONG_MAX_TERMS.
 *   enc32_out, xyzt_out (optional)    as d377_batch_msm_long's.
 * Any other index outside 0 .. pool_count - 1: the HOST form reads the whole n x m array before any copy or launch and
 * returns D377_ERR_ARG with a message that names point_index and the first offending position; no output byte is written.
 * The RESIDENT form cannot read its indices without a synchronisation: it walks such an index as an absent term, by an
 * unsigned compare, so nothing addresses past the pool, and when verdict != NULL a small kernel in front of the sums writes
 * the record of decaf377_amd_resident.h ("the index verdict"): verdict[0] = how many entries are neither -1 nor in
 * 0 .. pool_count - 1, verdict[1] = the first such position or UINT64_MAX.  A call with verdict[0] != 0 HAS PRODUCED the sums,
 * with those terms absent.
 * Arguments are checked in this order, all but the last two lines before any device is touched: m, pool_count (the message
 * names it), null pool_xyzt / point_index / scalar32 / enc32_out when n > 0, ctx; the resident form then dev and the
 * alignment (records 16 bytes, point_index 4, verdict 8); the host form then the indices.  n == 0 with good arguments is
 * D377_OK.  A multi-GPU context slices the SUMS over its devices and sends the pool to every device that gets a slice.
 * The sums are cut and folded as d377_batch_msm_long's (the same chains, table scratch, partial sums' area, fold and
 * compressor), with the point gathered through the index; m <= 8 runs the same kernels as one chain per sum.  The resident
 * form obeys the contract and the graph rules above.
 * Measured on one MI355X at 2^20 terms per call, (n, m) = (2^16, 16) / (2^12, 256) / (2^8, 4096), the legs of a pair
 * alternating in one process, median of 5 after 2 warm-ups with each leg's min-to-max spread
 * (profiles/msm_long_resident_bench.json, tools/bench_msm_long_resident.py; every leg timed to the end of a device synchronise):
 * the resident form 6.77 / 6.89 / 7.04 ms against 10.20 / 10.13 / 10.37 ms for the host form (spreads at most 0.17): USE THE
 * RESIDENT FORM for buffers on the device, it is ahead by more than both spreads.  The indexed host form over a pool of m
 * points shared by all sums 8.14 / 8.26 / 8.30 ms against 10.18 / 10.31 / 10.33 ms for d377_batch_msm_long on the materialised
 * array (spreads at most 0.22): USE THE INDEXED FORM where sums share their points.  The indexed resident form 6.58 / 6.70 /
 * 6.83 ms against 6.53 / 6.66 / 6.81 ms for the plain resident form on the materialised array (spreads 0.06 - 0.14): the cost of
 * the gather is NOT established; on device buffers the indexed form saves the n x m records' memory, not time. */
int d377_batch_long_msm_indexed(d377_ctx* ctx, const uint64_t* pool_xyzt, size_t pool_count, const int* point_index,
                                const uint8_t* scalar32, size_t m, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_batch_long_msm_indexed_resident(d377_ctx* ctx, int dev, void* stream, const uint64_t* pool_xyzt, size_t pool_count,
                                         const int* point_index, const uint8_t* scalar32, size_t m, size_t n, uint8_t* enc32_out,
                                         uint64_t* xyzt_out, uint64_t* verdict);

#ifdef __cplusplus
}
#endif
#endif /* DECAF377_AMD_LONG_SUMS_H */
