/*
 * decaf377_amd_resident.h -- the resident forms of the batched sums over registered bases: device pointers and a stream.
 * Included at the end of decaf377_amd.h, which declares everything these prototypes use; include that header.
 */
#ifndef DECAF377_AMD_RESIDENT_H
#define DECAF377_AMD_RESIDENT_H

#include "decaf377_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The batched sums over registered bases on DEVICE buffers: the resident forms.  Each takes the arguments of its host form preceded by
 * `int dev, void* stream`, with the semantics of the `_dev` family: every pointer is a device pointer resident on device
 * `dev` of the context; record buffers (points, Encodings, scalars, enc32_out, xyzt_out) are 16-byte aligned, base_index
 * 4-byte, verdict 8-byte -- anything else is D377_ERR_ARG; the call enqueues on `stream` (a hipStream_t, NULL = the default
 * stream) and returns, with no host synchronisation and no allocation once the scratch areas have grown to the shape; the
 * context's mutex is held while enqueuing; n == 0 with good arguments is D377_OK and enqueues nothing (no verdict record is
 * written either); starvation is the caller's check (d377_ctx_starved_counter_dev / d377_ctx_health, as documented for
 * `_dev`).  Arguments are checked in the host form's order with its texts: the ranges of v / t first, before ctx is
 * looked at, then null buffers when n > 0, ctx, and after those dev, the handle and the alignment.  The output bytes are
 * those of the host form on the same inputs.  d377_batch_sharded_dev does not take these operations.
 *   d377_batch_fixed_msm_resident            the combs are the handle's on device `dev`; on a handle of more than 64 bases
 *                                            it is d377_batch_fixed_long_msm_resident, as on the host.
 *   d377_batch_fixed_long_msm_resident       the cut is d377_fixed_long_msm_plan's for n sums on that device.
 *   d377_batch_fixed_msm_indexed_resident, d377_batch_msm_mixed[_encoded]_resident    see "the index verdict" below.
 * Graphs: the calls only enqueue kernels, so a sequence of them can be captured into a hipGraph and replayed.  The table
 * scratch and the partial sums' area cannot grow inside a stream capture (D377_ERR_ARG; nor can a kernel's residency be
 * asked for the first time): ONE EAGER CALL OF THE SHAPE MUST COME FIRST.  Once a launch on these areas has been captured, an
 * area that a later, larger call outgrows is kept until d377_ctx_destroy instead of freed, so an old graph stays valid.  A
 * replay that contains these calls must NOT overlap another batched-sum call of the same device on a different stream: the
 * table scratch's layout depends on the term count, and a capturing stream takes no part in the hand-over by events (order
 * them with the same stream or your own events).  Destroying a handle that a captured graph still names is the caller's
 * error.  The long variable-base sums' resident forms are in decaf377_amd_long_sums.h, under this contract.
 *
 * The index verdict.  The host forms of the indexed and mixed sums read every index before any launch; a resident call
 * cannot without a synchronisation.  Instead, when verdict != NULL, a small kernel in front of the sums kernel writes ONE
 * record per call, two u64 in device memory, initialised on the stream by the same call:
 *     verdict[0]   the number of entries of base_index that are neither -1 nor in 0 .. m-1
 *     verdict[1]   the position of the first such entry in the n x t array, or UINT64_MAX if there is none
 * verdict == NULL skips that kernel.  The resident contract for a refused index: it contributes nothing -- the sums kernels
 * walk it as an absent term, so no index can address past the combs -- and it is counted in the verdict.  A call whose
 * verdict[0] != 0 HAS PRODUCED the sums, with those terms absent, where the host form would have refused the whole call: a
 * caller reads the record once its stream has been synchronised and discards the outputs if it wants the host form's rule.
 * d377_check_base_index_resident runs the verdict alone over `count` indices (verdict must not be NULL; count == 0 gives
 * (0, UINT64_MAX)), for callers that want the host form's "nothing is computed": enqueue it, read the 16 bytes, launch
 * the sums only when verdict[0] == 0.
 * Measured on one MI355X against the host-pointer call of the same sums in the same process, the two alternating, median of 5
 * after 2 warm-ups with each leg's min-to-max spread (profiles/resident_sums_bench.json, tools/bench_resident_sums.py; the
 * resident leg is timed to the end of a device synchronise):  2^20 dense sums over one 18-bit base 1.13 ms against 4.66
 * (spreads 0.06 and 0.38), over three 16-bit bases 3.04 against 7.67 (0.12 and 0.25);
 * 2^12 mixed sums (1, 1, 1, 16) 1.07 against 1.15 (0.01 and 0.01).  USE THE RESIDENT FORM for those: it
 * is ahead by more than the two spreads.  NOT established at 2^20 indexed sums (64 bases, t = 2: 2.20 against 7.34 ms by the
 * medians, the host leg's spread 21.2 ms from one slow round) and at 2^20 mixed sums (1, 1, 1, 16) (16.9 against 24.6 ms, the
 * resident leg's spread 28.4 ms from one slow round).  The Encodings of the two legs were equal in every case.  The verdict
 * kernel alone takes 0.010 ms over the 2^21 indices of that indexed call: 0.45 % of it. */
int d377_batch_fixed_msm_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const uint8_t* scalar32, size_t n,
                                  uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_batch_fixed_long_msm_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const uint8_t* scalar32, size_t n,
                                       uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_batch_fixed_msm_indexed_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const int* base_index,
                                          const uint8_t* scalar32, size_t t, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out,
                                          uint64_t* verdict);
int d377_batch_msm_mixed_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const int* base_index,
                                  const uint8_t* fixed_scalar32, size_t t, const uint64_t* xyzt, const uint8_t* var_scalar32,
                                  size_t v, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out, uint64_t* verdict);
int d377_batch_msm_mixed_encoded_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const int* base_index,
                                          const uint8_t* fixed_scalar32, size_t t, const uint8_t* enc32,
                                          const uint8_t* var_scalar32, size_t v, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out,
                                          uint8_t* status, uint64_t* verdict);
int d377_check_base_index_resident(d377_ctx* ctx, int dev, void* stream, int64_t handle, const int* base_index, size_t count,
                                   uint64_t* verdict);

#ifdef __cplusplus
}
#endif
#endif /* DECAF377_AMD_RESIDENT_H */
