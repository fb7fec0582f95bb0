/*
 * decaf377_amd.h -- C ABI of the MI355X batch group-operation engine for decaf377.
 *
 * The reference crate (penumbra-zone/decaf377 v0.10.1) has no FFI or plugin interface of its
 * own (it is a #![no_std] Rust library, src/lib.rs:1-31); the boundary below is what a
 * Rust `extern "C"` block for this hot path would bind (INTEGRATION.md shows that block).
 * Every entry point is a pure map over packed, unpadded, element-major arrays: element i of
 * every output equals the reference function applied to element i of the inputs.
 *
 * Records
 *   Encoding   32 bytes, `Encoding(pub [u8; 32])`                 src/ark_curve/encoding.rs:14-15
 *   Fq / Fr    32 bytes little-endian                              src/fields/fq.rs:90-115, fr.rs:82-107
 *   Element    16 x u64 = X, Y, Z, T, each 4 Montgomery limbs (R = 2^256, fully reduced), the
 *              in-memory value of `Fq::from_montgomery_limbs`      src/fields/fq/u64/wrapper.rs:82-85
 *   status     1 byte per element: 0 = Ok, 1 = EncodingError::InvalidEncoding   src/error.rs:1-5
 *              (failed elements get all-zero output records)
 *
 * Return value: 0 on success, negative D377_ERR_* otherwise; per-element failures are only
 * reported through `status`.  Buffers belong to the caller and are never retained.  In place: in the element-wise
 * maps, d377_batch_* and d377_batch_*_dev and through d377_batch_sharded_dev, the output pointer may EQUAL the pointer
 * of any input whose records have the output's size -- the first input or the second (the scalars of scalar_mul_var,
 * r2 of hash_to_curve, the denominator of sqrt_ratio_zeta, b of the field operations), or both inputs at once; the status
 * buffer stays separate.  Until a call completes its output records may hold intermediate values.  Buffers that overlap
 * without being equal are not supported, and this sentence does not speak for the sums (d377_msm*, d377_batch_*msm*,
 * d377_sum_elements_dev), whose inputs and outputs differ in count.  Every such map runs in place on every launch route
 * in tests/test_in_place_gpu.py.
 *
 * Threads and streams.  Calls on one context are serialised by a mutex inside the context, so
 * several host threads may share it; distinct contexts are independent.  The `_dev` entry points
 * return as soon as the work is enqueued, and calls on DIFFERENT streams may be in flight at the
 * same time: the per-device scratch areas some kernels use (the variable-base window tables, the records of
 * the batched inversions behind scalar_mul_var / scalar_mul_base / encode_to_curve[_wide] / hash_to_curve /
 * sqrt_ratio_zeta, the Straus table scratch of the batched small, mixed, long and long-indexed sums, the partial-sums area
 * of the long, the long-indexed and the segmented fixed-base sums, the MSM workspace) are handed from one launch to the next
 * by events on the device, so such launches queue
 * up behind each other instead of racing -- results are the same as if the calls had been made one
 * after another; only their overlap is lost.  Kernels that use no scratch overlap freely.
 * There are two hand-overs per device.  One covers the lane-set areas, the table scratch and the partial-sums area: every
 * batched sum (d377_batch_msm_small*, d377_batch_msm_mixed*, d377_batch_long_msm*, d377_batch_fixed_*msm*) queues on it,
 * whatever its shape.  The other covers the MSM workspace, which d377_msm* and the bucket sums (d377_batch_bucket_msm*)
 * share: the two queue behind each other.  A call that outgrows an area waits on the host for the area's last user before
 * it frees it, d377_fixed_bases_destroy waits for the last launch on the combs, and a host-pointer call (the context's
 * private stream) queues behind `_dev` / `_resident` calls in flight like any other stream.
 * `_dev` calls only enqueue kernels (no host synchronisation, no allocation once the workspaces have grown
 * to the batch size), so a sequence of them can be captured into a hipGraph and replayed.  A capturing stream takes
 * no part in the event hand-over (the graph keeps its own order), so for a REPLAY that overlaps other calls on the same
 * device:
 *   - the lane-set areas (window tables, inversion records: every batch operation above) are safe -- each workgroup
 *     claims a free set atomically and nothing resets the pool between launches, so a replay and an eager call, or two
 *     replays, simply share them;
 *   - the MSM workspace is exclusive: do not let a replay that contains d377_msm*_dev overlap another MSM of the same
 *     device on a different stream (order them with the same stream or your own events);
 *   - a workspace never shrinks, and once an MSM has been captured an outgrown workspace is kept until
 *     d377_ctx_destroy instead of freed, so an old graph stays valid after later, larger calls; an MSM that would have
 *     to grow the workspace DURING a capture fails with D377_ERR_ARG (run one call of that size first).
 *
 * Three families:
 *   d377_batch_*          host pointers; the library copies to the context's GPU(s), shards
 *                         contiguous slices over them when the context owns several (one host
 *                         thread per device, so the devices run concurrently), and copies back.
 *   d377_batch_*_dev      device pointers (16-byte aligned, resident on the context's device
 *                         `dev`), enqueued on `stream` (a hipStream_t, NULL = default stream) with
 *                         no host synchronisation: for callers that keep batches in HBM.
 *   d377_batch_sharded_dev  a batch resident in the HBM of ONE device of a multi-GPU context:
 *                         contiguous slices go to the other devices by peer copies over xGMI, every
 *                         device runs the kernel, the outputs come back; ordered on `stream`.
 */
#ifndef DECAF377_AMD_H
#define DECAF377_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D377_OK 0
#define D377_ERR_HIP (-1)        /* a HIP runtime call failed; see d377_last_error() */
#define D377_ERR_ARG (-2)        /* null / misaligned pointer, bad device index */
#define D377_ERR_NO_DEVICE (-3)  /* no usable gfx950 device */
#define D377_ERR_INIT (-4)       /* device table self-check failed at context creation */
#define D377_ERR_STARVED (-5)    /* workgroups of this call found no free lane set for 10 s and wrote no output: the
                                    output buffers are NOT valid (d377_ctx_health, d377_ctx_reset_scratch below) */

typedef struct d377_ctx d377_ctx;

/* Library / device discovery. */
const char* d377_version(void);
int d377_device_count(void);
/* Human-readable text for the most recent error on this thread. */
const char* d377_last_error(void);

/* Builds the read-only device tables (Sarkar square-root tables of
 * src/ark_curve/invsqrt.rs:14-66, fixed-base table of Element::GENERATOR) once per device
 * and allocates the per-device scratch (about 6.7 GB of HBM per device: 0.73 GB of window tables and records of the
 * batched inversions, and the 5.9 GB fixed-base comb of 23-bit windows, built in 16 ms).  device_ids == NULL,
 * n_dev == 0 -> device 0.  The comb is the one cost a caller may not want: in the reference Element::GENERATOR is a
 * constant (src/min_curve/element.rs:61-81) and `GENERATOR * Fr` costs nothing until it is used -- d377_ctx_create_ex
 * makes it so here too. */
int d377_ctx_create(const int* device_ids, int n_dev, d377_ctx** out);
/* The same with options (NULL = d377_ctx_create's defaults).
 *   size        sizeof(d377_ctx_opts) as the caller was compiled (fields added later default to 0)
 *   comb_bits   width of the fixed-base comb: 0 = the library's default (23), or 18 / 21 / 23 --
 *               0.24 / 1.6 / 5.9 GB per device, 14 / 12 / 11 additions per scalar (18 is 9-12 % slower than 23 on
 *               d377_batch_scalar_mul_base*, profiles/r05_ab_fixed_base_wide.txt); results are the same bytes
 *   comb_lazy   0: the comb is built at context creation.  1: by the first fixed-base call on each device
 *               (d377_batch_scalar_mul_base[_element][_dev], d377_batch_sharded_dev with those operations), which then
 *               allocates, builds (16 ms at 23 bits) and synchronises once -- so that first call must not be inside a
 *               stream capture (D377_ERR_ARG); a context that never multiplies by the generator holds 0.73 GB per device.
 * A failed comb allocation is D377_ERR_HIP with a text that names the width and the smaller ones.
 * d377_ctx_comb_info: the width of device `dev`'s comb, whether it has been built, and its size in bytes (any pointer
 * may be NULL). */
typedef struct d377_ctx_opts {
  size_t size;
  int comb_bits;
  int comb_lazy;
} d377_ctx_opts;
int d377_ctx_create_ex(const int* device_ids, int n_dev, const d377_ctx_opts* opts, d377_ctx** out);
int d377_ctx_comb_info(d377_ctx* ctx, int dev, int* comb_bits, int* built, uint64_t* table_bytes);
void d377_ctx_destroy(d377_ctx* ctx);
int d377_ctx_num_devices(const d377_ctx* ctx);
int d377_ctx_device_id(const d377_ctx* ctx, int dev);
/* What d377_ctx_create arranged between two devices of the context: 2 = they are distinct GPUs and peer access
 * dev_a -> dev_b (xGMI) was enabled, 1 = the same physical GPU listed twice, 0 = distinct GPUs without peer access
 * (d377_batch_sharded_dev then relies on the runtime's staged copies), -1 = bad index. */
int d377_ctx_peer_access(const d377_ctx* ctx, int dev_a, int dev_b);
/* The lane-set scratch areas hold `sets_per_cu` sets per compute unit (3: the fixed-base kernel claims among all of
 * them, the other kernels among the first 2 per CU); d377_ctx_create asks the runtime
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor) how many workgroups of each kernel that claims a set can be resident
 * per CU, pads a kernel's launch with dynamic LDS when its registers alone would admit more than the sets it may claim,
 * and fails with D377_ERR_INIT if one still exceeds them.  Reports the numbers it settled on: the largest residency over those
 * kernels (<= sets_per_cu) and the largest LDS padding in use (0 when none was needed).  Any pointer may be NULL. */
int d377_ctx_chunk_residency(const d377_ctx* ctx, int dev, int* sets_per_cu, int* max_blocks_per_cu, int* lds_pad_bytes);
/* The lane-set pool's health and its way back.  Every workgroup of a chunked kernel claims one lane set of the scratch
 * areas and frees it when it is done; a launch that dies mid-kernel (a fault in another kernel of the process, a killed
 * graph) would leave its sets claimed for the life of the context.  Later launches then wait: a workgroup that finds
 * no free set for 0.25 s is counted in *waited_long and keeps waiting; after 10 s it is counted in *gave_up and leaves
 * WITHOUT writing its output records (so no launch can spin forever).  That is never a silent wrong answer -- the
 * reference's fallible operations always return a Result (src/ark_curve/encoding.rs:34-60):
 *   - every host-pointer entry point (d377_batch_*, d377_msm[_encoded]) reads the gave-up counter on its stream before
 *     its first and after its last kernel and returns D377_ERR_STARVED when it moved; the output buffers are then invalid;
 *   - a `_dev` call only enqueues, so its caller checks: d377_ctx_starved_counter_dev gives the DEVICE address of the
 *     32-bit counter (valid for the life of the context, only ever incremented); copy it on the call's stream before and
 *     after the call (two 4-byte copies, no synchronisation of their own) and compare once the stream has been
 *     synchronised, or call d377_ctx_health afterwards.  Either check is MANDATORY after any `_dev` call that took
 *     longer than 10 s before its outputs are trusted; a call that finishes sooner cannot have starved.
 * d377_ctx_health reports the sets claimed right now (0 on an idle device) and both counters since the context was created; it
 * does not wait for running kernels.  d377_ctx_reset_scratch frees leaked sets: it reads the pool, waits for the work
 * this context knows of (at least 0.25 s, at most 1.5 s), reads it again and frees exactly the sets whose ticket did
 * not change in between -- a workgroup draws a new ticket for every chunk it starts (milliseconds of work), so a
 * ticket that stood still belongs to no running workgroup, however long its launch and whether or not the context can
 * see it (a replayed hipGraph) -- then waits for starved work to finish.  *sets_released (may be NULL) = how many it
 * freed; 0 on a healthy context.
 * d377_debug_poison_pool marks `sets` sets (< 0: all) as claimed by nobody: the test hook for the calls above. */
int d377_ctx_health(d377_ctx* ctx, int dev, int* sets_claimed, uint64_t* waited_long, uint64_t* gave_up);
int d377_ctx_reset_scratch(d377_ctx* ctx, int dev, int* sets_released);
int d377_ctx_starved_counter_dev(d377_ctx* ctx, int dev, const uint32_t** counter_dev);
int d377_debug_poison_pool(d377_ctx* ctx, int dev, int sets);
/* Debug builds (-DD377_CHECK_INVARIANTS, the counterpart of the reference's debug assertions in
 * Element::new, src/min_curve/element.rs:104-110, and is_on_curve, src/ark_curve/on_curve.rs:14-39): how many
 * group elements failed the curve equation / T Z = X Y / Z != 0 after decompression, the Elligator map or on
 * their way into compression since the context was created.  Synchronises the device.  Returns 1 when the
 * checks are compiled in, 0 (and *count = 0) in a normal build, negative on error. */
int d377_ctx_invariant_failures(d377_ctx* ctx, int dev, uint64_t* count);

/* Developer interface: launch-rule overrides.  The library picks kernels, chunk shapes and MSM parameters from the
 * batch size and the device's CU count; these keys replace one rule each for A/B measurements and for tests that force
 * a route over sizes that would not take it (every route gives the same bytes).  Values are validated, stored in the
 * context, and read under its mutex by every later call on it (calls already enqueued keep what they were launched
 * with); D377_TUNE_DEFAULT restores the built-in rule.  Nothing in the library reads the process environment on a call
 * path (D377_DEBUG_* diagnostics at context creation and in the multi-device test hook aside).
 *   SMALL_MAX              scalar_mul_var[_element], scalar_mul_base[_element]: batches up to this many elements take the quad-per-element
 *                          kernel (0 = never; it also caps TINY_MAX)
 *   DECOMPRESS_CHUNKED_MIN decompress, compress, roundtrip: batches from this many elements run in chunks with shared inversions
 *   FB_WIDE                scalar_mul_base: 0 = narrow launch (2 workgroups per CU), 1 = wide (3 per CU) at every size the lane kernel takes
 *   FB_K                   scalar_mul_base: elements per lane per shared inversion, 1..16
 *   AFFINE_BLOCKS_PER_CU   to_affine: workgroups per CU that share the batch, >= 1
 *   MSM_WINDOW             msm: window width in bits, 4..18
 *   MSM_SEG                msm: sorted entries per span lane, 1..128 (built-in: entries / resident lanes, at least 8)
 *   MSM_SMALL_MAX          msm: batches up to this many points skip the buckets (0 = never)
 *   MSM_SLICES             msm: slices per window of the counting sort, 1..4096
 *   MSM_SORT_PACKED        msm: 0 = the sort's level-1 entries as a word and a byte (the form batches above 2^24 points take), 1 = one
 *                          packed word (refused above 2^24 points)
 *   MSM_RED / MSM_SKIP     msm: group size of the second reduction level (2..64) / leftovers a bucket lane sums itself (1..64)
 *   MSM_CHUNKED_SUMS       msm: 1 = weighted bucket sums by chunked running sums instead of the tree of bit-sums
 *   MSM_ENC_CHUNKED_MIN    msm_encoded: batches from this many points decode with shared inversions
 *   TINY_MAX               scalar_mul_var[_element], scalar_mul_base[_element]: batches up to this many elements take one wave per
 *                          element (0 = never); sqrt_ratio_zeta, decompress, compress, roundtrip, encode_to_curve, hash_to_curve:
 *                          batches up to FOUR times this many take four elements per wave (hash_to_curve up to twice: two pairs)
 *   MSM_TINY_MAX           msm: batches up to this many points take a wave per one to four points (0 = never; at most MSM_SMALL_MAX applies)
 *   CHUNK_PER_LANE         chunked kernels (sqrt_ratio_zeta, encode_to_curve[_wide], hash_to_curve, scalar_mul_var): elements per lane per chunk, 1..8
 * Returns D377_ERR_ARG for an unknown key or a value outside its range. */
#define D377_TUNE_SMALL_MAX 0
#define D377_TUNE_DECOMPRESS_CHUNKED_MIN 1
#define D377_TUNE_FB_WIDE 2
#define D377_TUNE_FB_K 3
#define D377_TUNE_AFFINE_BLOCKS_PER_CU 4
#define D377_TUNE_MSM_WINDOW 5
#define D377_TUNE_MSM_SEG 6
#define D377_TUNE_MSM_SMALL_MAX 7
#define D377_TUNE_MSM_SLICES 8
#define D377_TUNE_MSM_RED 9
#define D377_TUNE_MSM_SKIP 10
#define D377_TUNE_MSM_CHUNKED_SUMS 11
#define D377_TUNE_MSM_ENC_CHUNKED_MIN 12
#define D377_TUNE_CHUNK_PER_LANE 13
#define D377_TUNE_MSM_TINY_MAX 14
#define D377_TUNE_TINY_MAX 15
#define D377_TUNE_MSM_SORT_PACKED 16
#define D377_TUNE_COUNT 17
#define D377_TUNE_DEFAULT (-1)
int d377_ctx_set_tuning(d377_ctx* ctx, int key, int64_t value);
int d377_ctx_get_tuning(d377_ctx* ctx, int key, int64_t* value);

/* Fq::sqrt_ratio_zeta(num, den) -> (was_square, root)        src/ark_curve/invsqrt.rs:75-166
 * num32/den32: 32-byte strings reduced mod q like Fq::from_le_bytes_mod_order.
 * The crate's two backends return different roots (same flag, root negated about half the time):
 *   D377_SQRT_ROOT_ARK        the default `arkworks` backend, Sarkar's table method   src/ark_curve/invsqrt.rs:75-166
 *   D377_SQRT_ROOT_MIN_CURVE  `Fq::non_arkworks_sqrt_ratio_zeta`, constant-time Tonelli-Shanks seeded
 *                             with 11^m                       src/min_curve/invsqrt.rs:11-95, src/fields/fq.rs:62-67
 * d377_batch_sqrt_ratio_zeta returns the ARK root; the _ex forms take the convention.  Every group-level
 * output (encodings) is the same under either: decompress / compress / Elligator fix the sign themselves. */
#define D377_SQRT_ROOT_ARK 0
#define D377_SQRT_ROOT_MIN_CURVE 1
int d377_batch_sqrt_ratio_zeta(d377_ctx* ctx, const uint8_t* num32, const uint8_t* den32, size_t n,
                               uint8_t* root32, uint8_t* was_square);
int d377_batch_sqrt_ratio_zeta_ex(d377_ctx* ctx, int root, const uint8_t* num32, const uint8_t* den32, size_t n,
                                  uint8_t* root32, uint8_t* was_square);
/* Encoding::vartime_decompress                                src/ark_curve/encoding.rs:32-83 */
int d377_batch_decompress(d377_ctx* ctx, const uint8_t* enc32, size_t n, uint64_t* xyzt, uint8_t* status);
/* Element::vartime_compress                                   src/ark_curve/encoding.rs:91-128 */
int d377_batch_compress(d377_ctx* ctx, const uint64_t* xyzt, size_t n, uint8_t* enc32);
/* vartime_decompress then vartime_compress (tests/encoding.rs:97-107 round trip) */
int d377_batch_roundtrip(d377_ctx* ctx, const uint8_t* enc32, size_t n, uint8_t* enc32_out, uint8_t* status);
/* Element::GENERATOR * Fr::from_le_bytes_mod_order(scalar) -> Encoding
 *                                                             src/min_curve/ops.rs:89-95 */
int d377_batch_scalar_mul_base(d377_ctx* ctx, const uint8_t* scalar32, size_t n, uint8_t* enc32_out);
/* Encoding::vartime_decompress(enc)? * Fr::from_le_bytes_mod_order(scalar) -> Encoding */
int d377_batch_scalar_mul_var(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, size_t n,
                              uint8_t* enc32_out, uint8_t* status);
/* Element::encode_to_curve(Fq::from_le_bytes_mod_order(r)) -> Encoding
 *                                                             src/ark_curve/elligator.rs:15-62,74-76 */
int d377_batch_encode_to_curve(d377_ctx* ctx, const uint8_t* fq32, size_t n, uint8_t* enc32_out);
/* Element::hash_to_curve(r1, r2) -> Encoding                  src/ark_curve/elligator.rs:67-71 */
int d377_batch_hash_to_curve(d377_ctx* ctx, const uint8_t* r1_32, const uint8_t* r2_32, size_t n,
                             uint8_t* enc32_out);

/* The same operations with the reference's own signatures: Elements in, Elements out, no encoding step.
 *   Element * Fr                                               src/min_curve/ops.rs:89-95, element.rs:138-157
 *   Element::GENERATOR * Fr
 *   Element::vartime_compress_to_field -> Fq (4 Montgomery limbs) src/min_curve/element.rs:163-181
 *   Element::encode_to_curve / hash_to_curve -> Element         src/min_curve/element.rs:190-244
 * An Element returned by the scalar multiplications is some extended representative of the reference's group
 * element (same encoding, equal under d377_batch_eq); its X:Y:Z:T are those of the schedule here (signed
 * windows), not of the reference's double-and-add.  encode_to_curve / hash_to_curve return the coordinates
 * the reference's formulas give.  scalar32: any 32 bytes, reduced mod r. */
int d377_batch_scalar_mul_var_element(d377_ctx* ctx, const uint64_t* p_xyzt, const uint8_t* scalar32, size_t n,
                                      uint64_t* out_xyzt);
int d377_batch_scalar_mul_base_element(d377_ctx* ctx, const uint8_t* scalar32, size_t n, uint64_t* out_xyzt);
int d377_batch_compress_to_field(d377_ctx* ctx, const uint64_t* p_xyzt, size_t n, uint64_t* fq_out);
int d377_batch_encode_to_curve_element(d377_ctx* ctx, const uint8_t* fq32, size_t n, uint64_t* out_xyzt);
int d377_batch_hash_to_curve_element(d377_ctx* ctx, const uint8_t* r1_32, const uint8_t* r2_32, size_t n,
                                     uint64_t* out_xyzt);

/* Element + Element, Element - Element (= self + other.neg()), Element::double, decaf equality
 * (x1*y2 == x2*y1) on in-memory elements
 *            src/min_curve/element.rs:291-322, 119-136, 334-340; src/min_curve/ops.rs:15-87;
 *            ark: element/projective.rs:65-70
 * Results are the same extended coordinates the reference formulas produce. */
int d377_batch_add(d377_ctx* ctx, const uint64_t* p_xyzt, const uint64_t* q_xyzt, size_t n, uint64_t* out_xyzt);
int d377_batch_sub(d377_ctx* ctx, const uint64_t* p_xyzt, const uint64_t* q_xyzt, size_t n, uint64_t* out_xyzt);
int d377_batch_double(d377_ctx* ctx, const uint64_t* p_xyzt, size_t n, uint64_t* out_xyzt);
int d377_batch_eq(d377_ctx* ctx, const uint64_t* p_xyzt, const uint64_t* q_xyzt, size_t n, uint8_t* equal);

/* Fq::from_le_bytes_mod_order on 48- or 64-byte strings (hash outputs)      src/fields/fq.rs:90-102
 * -> canonical 32-byte Fq; and the same fused into encode_to_curve.  len must be 48 or 64. */
int d377_batch_fq_from_wide_bytes(d377_ctx* ctx, const uint8_t* bytes, size_t len, size_t n, uint8_t* fq32_out);
int d377_batch_encode_to_curve_wide(d377_ctx* ctx, const uint8_t* bytes, size_t len, size_t n, uint8_t* enc32_out);
/* CurveGroup::normalize_batch / into_affine                                   src/ark_curve/element.rs:74-85
 * xy: n x 8 u64 = affine x, y as 4 Montgomery limbs each. */
int d377_batch_to_affine(d377_ctx* ctx, const uint64_t* xyzt, size_t n, uint64_t* xy);

/* Element::vartime_multiscalar_mul(scalars, points) = sum_i scalar_i * point_i
 *                                                 src/ark_curve/element/projective.rs:99-117
 * (a fold of scalar multiplications in the reference; here a Pippenger bucket MSM, and for batches small enough to
 * give every point four lanes -- up to 64 per compute unit, 16384 on an MI355X -- one scalar multiplication per point
 * followed by a tree sum).  The sum is returned as its canonical Encoding (enc32_out, 32 bytes) and, if xyzt_out !=
 * NULL, as one Element record (some extended representative of the same group element).  Element records are read
 * as the extended coordinates they are (T Z = X Y, as every Element the reference or this library produces has
 * them); a record with Z = 0 is no group element and counts as the identity.
 * d377_msm takes in-memory Elements; d377_msm_encoded takes Encodings, reports invalid ones in
 * status[] and leaves them out of the sum.  n < 2^31.  With a multi-GPU context each device sums a
 * contiguous slice and the partial sums are added on the first device. */
int d377_msm(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalar32, size_t n, uint8_t* enc32_out,
             uint64_t* xyzt_out);
int d377_msm_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, size_t n, uint8_t* enc32_out,
                     uint64_t* xyzt_out, uint8_t* status);

/* MANY small multiscalar sums at once: sum i = scalar[i m] * point[i m] + ... + scalar[i m + m - 1] * point[i m + m - 1] for
 * i < n, m terms per sum, 1 <= m <= D377_BATCH_MSM_MAX_TERMS; enc32_out[i] = the canonical Encoding of sum i and, if
 * xyzt_out != NULL, xyzt_out[i] = sum i as an Element record (n x 16 u64; some extended representative, as d377_msm's).  This is
 * Element::vartime_multiscalar_mul (src/ark_curve/element/projective.rs:99-117) in the shape the reference's own test
 * exercises it -- a 3-term sum per case, tests/operations.rs:44-60 -- for callers that hold many such sums (d377_msm is ONE
 * long sum per call).  Each sum is one Straus chain: its m points share the 252 doublings, so a 3-term sum costs about half
 * of three scalar multiplications and two additions.  Points and scalars are term-major within a sum: n x m records each.
 * d377_batch_msm_small takes Elements (read as the extended coordinates they are, T Z = X Y; a record with Z = 0 counts as
 * the identity); _encoded takes Encodings, reports invalid ones in status[i m + j] (n x m bytes) and leaves them out of
 * their sum, like d377_msm_encoded.  Scratch: 0.23 GB of HBM per term on a 256-CU device, allocated on the first call
 * with that many terms (so that call must not be inside a stream capture).  A multi-GPU context slices the SUMS. */
#define D377_BATCH_MSM_MAX_TERMS 8
int d377_batch_msm_small(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalar32, size_t m, size_t n, uint8_t* enc32_out,
                         uint64_t* xyzt_out);
int d377_batch_msm_small_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, size_t m, size_t n,
                                 uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status);

/* MANY multiscalar sums of medium length at once: the same sums as d377_batch_msm_small[_encoded], with
 * 1 <= m <= D377_BATCH_MSM_LONG_MAX_TERMS terms per sum -- Pedersen vector commitments to a thousand vectors of 256 entries,
 * the rounds of an inner-product argument, many batches of verification equations.  The semantics are exactly those of the
 * small sums: points and scalars are n x m records, term-major within a sum; enc32_out[i] = the canonical Encoding of sum i;
 * xyzt_out (optional) = the sums as Element records (some extended representative); _encoded reports invalid Encodings in
 * status[i m + j] and leaves them out of their sum; a record with Z = 0 counts as the identity; scalars are any 32 bytes,
 * reduced mod r.  The length is UNIFORM: a caller with shorter sums pads them with zero scalars or Z = 0 records, which
 * contribute nothing (and cost as much as a present term).
 * Cost model: a sum is cut into g = ceil(m / 8) groups of b = ceil(m / g) terms, each group is one Straus chain of the small
 * sums (252 doublings + 64 b additions + b tables), and the g partial sums are added on the device, 16 per lane and level
 * (at most three levels), before ONE compressor pass, no host round trips (by instruction count, an estimate that was not
 * measured: about 8 % more than m / 8 eight-term chains).  Up to four chains per SIMD run a wave each, beyond that a lane each.
 * Measured on one MI355X, host arrays, 2^20 terms per call (profiles/batch_msm_long_bench.json): 10.2 ms at (n, m) =
 * (2^16, 16), (2^12, 256) and (2^8, 4096) alike, against 18.1 / 21.7 / 21.9 ms for the composition through host memory
 * (d377_batch_msm_small on groups of 8, rounds of d377_batch_add, d377_batch_compress: x 1.8 / 2.1 / 2.1) and 18.4 s / 1.34 s /
 * 123 ms for n calls of d377_msm (scaled from 128 calls).  For m <= 8 the call forwards to d377_batch_msm_small[_encoded] (the
 * same bytes).  For ONE long sum use d377_msm: measured at (1, 4096), 0.97 ms here against 0.48 ms for d377_msm (the
 * composition: 1.31 ms) -- a single sum is 512 chains on 512 waves of a chip that holds thousands, as long as one chain plus
 * three fold levels and a compressor pass, while the Pippenger MSM needs fewer additions (by count about a third: an
 * estimate).  Scratch: the small sums' table scratch for b terms, and 128 bytes per group, grown on demand and kept (a failed
 * allocation is D377_ERR_HIP and leaves nothing half-allocated).
 * Arguments are checked in this order, the first two before any device is touched: m (0 or more than 4096 is D377_ERR_ARG,
 * the message names m), null buffers when n > 0, ctx; n == 0 with good arguments is D377_OK.  A multi-GPU context slices the
 * SUMS over its devices.  Device buffers take d377_batch_long_msm[_encoded]_resident, and sums whose terms name their points
 * in a shared pool d377_batch_long_msm_indexed[_resident]: decaf377_amd_long_sums.h, which this header includes at its end. */
#define D377_BATCH_MSM_LONG_MAX_TERMS 4096
int d377_batch_msm_long(d377_ctx* ctx, const uint64_t* xyzt, const uint8_t* scalar32, size_t m, size_t n, uint8_t* enc32_out,
                        uint64_t* xyzt_out);
int d377_batch_msm_long_encoded(d377_ctx* ctx, const uint8_t* enc32, const uint8_t* scalar32, size_t m, size_t n,
                                uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status);

/* Fixed-base combs for caller-chosen points, and many sums over them.  The reference reaches this through arkworks:
 * Element implements ScalarMul / VariableBaseMSM / CurveGroup (src/ark_curve/element.rs:22-38), so ark-ec's FixedBase
 * window tables work on any Element -- a Pedersen commitment v G + r H, a value commitment's asset and blinding generators.
 *
 * d377_fixed_bases_create registers 1 <= m <= D377_FIXED_BASES_MAX bases (m x 16 u64 Element records, read as the extended
 * coordinates they are, T Z = X Y; a record with Z = 0 counts as the identity) and builds one comb per base on every device
 * of the context: window i of base j holds c * 2^(comb_bits i) * B_j for 0 <= c <= 2^(comb_bits - 1).  comb_bits: 8, 12,
 * 16 or 18 (0 = 16); per base 0.53 MB / 5.5 MB / 67 MB / 235 MB of HBM and 32 / 21 / 16 / 14 mixed additions per sum.
 * m, comb_bits and the pointers are checked before any device is touched (D377_ERR_ARG, the message names the argument);
 * tables that do not fit fail with D377_ERR_HIP and leave nothing allocated.  The context's own generator comb
 * (d377_ctx_create_ex) is independent of these.
 *
 * d377_batch_fixed_msm computes n sums, enc32_out[i] = the canonical Encoding of
 *     scalar[i m] * B_0 + ... + scalar[i m + m - 1] * B_{m-1}
 * (scalars term-major within a sum, n x m 32-byte strings, any 32 bytes, reduced mod r) and, if xyzt_out != NULL, the
 * sums as Element records (n x 16 u64, some extended representative: equal under d377_batch_eq, same encoding).  Any
 * representative of a base gives the same encodings, one that differs by a torsion point the encoding quotients away
 * included.  m = 1 is a fixed-base multiplication by B_0.  A multi-GPU context slices the SUMS over its devices.
 * The host-pointer form; device buffers take d377_batch_fixed_msm_resident (decaf377_amd_resident.h).
 *
 * d377_batch_fixed_msm_indexed computes n sums of t terms each, 1 <= t <= D377_FIXED_BASES_MAX, whose terms name their
 * bases: enc32_out[i] = the canonical Encoding of
 *     sum over j < t of  scalar[i t + j] * B_{base_index[i t + j]}
 * (base_index n x t ints and scalar32 n x t 32-byte strings, both term-major within a sum; xyzt_out as above).  An index
 * is a base's position in the registration, 0 .. m-1; the same index may appear several times in one sum, and the terms
 * add.  -1 means "this term is absent": it contributes nothing and its scalar bytes are ignored, which is how sums with
 * fewer than t terms are written -- but an absent term COSTS AS MUCH AS A PRESENT ONE (it walks the identity entries of a
 * comb), so t should be the longest sum's length, not m.  A sum whose terms are all absent is the identity (the all-zero
 * Encoding).  Any other index (< -1 or >= m) is D377_ERR_ARG: the whole n x t array is checked on the host before any
 * copy or launch, the message names base_index and the first offending position, and no output is written.  Arguments
 * are checked in this order: t, null base_index / scalar32 / enc32_out (n > 0), ctx, the handle, the indices; n == 0 with
 * good arguments is D377_OK.  With 64 registered bases a two-term sum is 2 W mixed additions where the dense call walks
 * 64 W and uploads 64 scalars.  The host-pointer form, sliced over the devices of a multi-GPU context by SUMS, as above; device
 * buffers take d377_batch_fixed_msm_indexed_resident (decaf377_amd_resident.h), which answers the indices with a verdict record.
 *
 * Handles: a handle is a positive integer that names one registration within its context (never reused by that
 * context); every call takes the context and the handle, and a handle that was destroyed, or never created there, is
 * refused with D377_ERR_ARG.  Threads and lifetime: calls on one handle, or on several handles of one context, may come
 * from several host threads; they are serialised by the context's mutex like every host-pointer call.  Handles are
 * destroyed before their context; d377_ctx_destroy releases the tables of any handle still alive.  The C++ and Python
 * wrappers keep that order themselves.  d377_fixed_bases_info reports m, the comb width and the table bytes per device.
 *
 * Long registrations and long sums -- Pedersen vector commitments over hundreds or thousands of generators, the rounds of an
 * inner-product argument, a value commitment that names its asset generator among thousands.
 * d377_fixed_bases_create_long is d377_fixed_bases_create with 1 <= m <= D377_FIXED_BASES_LONG_MAX = 4096 bases and
 * comb_bits 0 = 12: the same records (Z = 0 is the identity), the same build, handles of the same registry (d377_fixed_bases_info
 * / _destroy, release with the context), the same checks in the same order -- m, comb_bits, xyzt, handle_out, ctx, all before
 * any device is touched.  4096 bases are 2.2 GB at 8 bits and 22.5 GB at 12; tables that do not fit fail with D377_ERR_HIP,
 * the message names the gigabytes, and nothing stays allocated.  d377_fixed_bases_create keeps its limit of 64.
 *
 * d377_batch_fixed_long_msm computes the sums of d377_batch_fixed_msm -- the same semantics, scalar reduction, argument checks
 * and slicing of the SUMS over the devices -- on ANY live handle, short or long, with every sum cut into g segments of
 * b consecutive bases, one GPU lane per segment: where d377_batch_fixed_msm gives a sum one lane (a thousand sums of 256 bases
 * are a thousand lanes of a chip that holds 131 072), the cut fills the chip.  With L the device's resident lanes,
 *     g0 = min(m, ceil(L / n)),  b = ceil(m / g0),  g = ceil(m / b)
 * (b one less where rounding it up would leave the chip short by more than one segment per sum); the segments' partial sums
 * are folded on the device, 16 records per lane and level, and compressed in one pass, as d377_batch_msm_long's are.
 * n >= L or m = 1 is one segment per sum: d377_batch_fixed_msm's kernel and bytes.  d377_fixed_long_msm_plan reports g
 * (`segments`) and b (`bases_per_segment`) for the slice device `dev` of the context gets of a call of n sums (0 and 0 where it
 * gets none); it is pure and cheap and takes the context's mutex.  d377_batch_fixed_msm on a handle of more than 64 bases IS
 * d377_batch_fixed_long_msm.  d377_batch_fixed_msm_indexed takes long handles as they are: indices 0 .. m-1 or -1, t <= 64.
 * Against d377_batch_msm_long on the same sums (the m points replicated n times: 160 bytes uploaded per term instead of 32, a
 * window table per copy, 252 doublings per chain and 64 additions per term) a term is 21 mixed additions at 12 bits and
 * nothing else.  Measured (profiles/fixed_msm_long_bench.json, tools/bench_fixed_msm_long.py; host path): 2^12 sums of 256
 * bases at 12 bits 2.23 ms against 10.61 ms, 2^8 sums of 4096 bases 2.32 ms against 10.67 ms (12 bits, 22.5 GB of combs) and
 * 2.99 against 10.81 (8 bits), 2^16 sums of 65 bases 8.08 against 43.10; the kernel walks 1.70e10 additions per second over
 * 22.5 GB of combs as over 2.2 GB.  256 sums over a 64-base handle: 0.39 ms against 3.64 ms through d377_batch_fixed_msm.
 * For ONE sum use d377_msm: 0.45 ms against 0.60 ms at 4096 terms.  Device buffers: d377_batch_fixed_long_msm_resident. */
#define D377_FIXED_BASES_MAX 64
#define D377_FIXED_BASES_LONG_MAX 4096
int d377_fixed_bases_create(d377_ctx* ctx, const uint64_t* xyzt, size_t m, int comb_bits, int64_t* handle_out);
int d377_fixed_bases_info(d377_ctx* ctx, int64_t handle, uint64_t* m, int* comb_bits, uint64_t* table_bytes_per_device);
int d377_fixed_bases_destroy(d377_ctx* ctx, int64_t handle);
int d377_batch_fixed_msm(d377_ctx* ctx, int64_t handle, const uint8_t* scalar32, size_t n, uint8_t* enc32_out,
                         uint64_t* xyzt_out);
int d377_batch_fixed_msm_indexed(d377_ctx* ctx, int64_t handle, const int* base_index, const uint8_t* scalar32, size_t t,
                                 size_t n, uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_fixed_bases_create_long(d377_ctx* ctx, const uint64_t* xyzt, size_t m, int comb_bits, int64_t* handle_out);
int d377_batch_fixed_long_msm(d377_ctx* ctx, int64_t handle, const uint8_t* scalar32, size_t n, uint8_t* enc32_out,
                              uint64_t* xyzt_out);
int d377_fixed_long_msm_plan(d377_ctx* ctx, int64_t handle, size_t n, int dev, uint64_t* segments,
                             uint64_t* bases_per_segment);

/* MANY mixed sums at once: registered bases plus variable points in one sum.  enc32_out[i] = the canonical Encoding of
 *     sum over j < t of  fixed_scalar[i t + j] * B_{base_index[i t + j]}   +   sum over p < v of  var_scalar[i v + p] * P[i v + p]
 * with 1 <= t <= D377_FIXED_BASES_MAX terms among the bases of `handle` and 1 <= v <= D377_BATCH_MSM_MIXED_MAX_VAR points of the
 * sum's own: the check of a signature or a sigma protocol, R' = s B - c A (t = v = 1: what other curve libraries offer as
 * vartime_double_scalar_mul_basepoint), and a commitment with an opening, v G_asset + r H + sum k_p P_p.  Every rule of
 * d377_batch_fixed_msm_indexed holds for the fixed half and every rule of d377_batch_msm_small[_encoded] for the variable
 * half: base_index is n x t ints, fixed_scalar32 n x t and var_scalar32 n x v 32-byte strings, the points n x v Element
 * records (xyzt) or Encodings (enc32), all term-major within a sum; scalars are any 32 bytes, reduced mod r; index -1 is an
 * absent term, which COSTS AS MUCH AS A PRESENT ONE; an index may repeat within a sum; any live handle works, short or long,
 * with indices 0 .. m-1; an Element record with Z = 0 counts as the identity; _encoded reports an invalid Encoding in
 * status[i v + p] and leaves only that term out; xyzt_out (optional) = the sums as Element records (some extended
 * representative).  For t = 0 use d377_batch_msm_small, for v = 0 d377_batch_fixed_msm_indexed.
 * One GPU lane computes a whole sum: the Straus chain of the small sums over its v points (252 doublings + 64 v additions +
 * v tables), the comb walk of the indexed sums over its t terms (14-32 mixed additions each, no doubling), one addition that
 * joins the two halves and one pass of the square-root-free compressor.  There is no wave-per-sum route: a small batch is
 * as long as one chain.  Composed of existing calls the same sum is d377_batch_msm_small and d377_batch_fixed_msm_indexed
 * with Element output, d377_batch_add and d377_batch_compress: four calls, and 128-byte records through host memory after
 * each of the first three.
 * Measured on one MI355X, host arrays, against that four-call composition in the same process, the two alternating, median of 5
 * after 2 warm-ups with the min-to-max spread of each (profiles/msm_mixed_bench.json, tools/bench_msm_mixed.py), shapes
 * (v, t, bases, comb_bits):  2^20 sums of (1, 1, 1, 16), the signature check: 25.3 ms against 117.6 ms (x 4.6; spreads 30.4 and
 * 53.2 ms, one slow round each);  2^20 of (1, 2, 64, 16): 27.6 against 116.2 ms (x 4.2; spreads 27.5 and 50.8);  2^12 of the same
 * two: 1.14 against 1.33 ms and 1.20 against 1.38 ms (x 1.17 and x 1.15; spreads below 0.09 ms).  USE THIS CALL for those: it is
 * ahead by more than the two spreads.  For (3, 2, 64, 12) it is NOT established: 44.7 against 129.5 ms at 2^20 (x 2.9 by the
 * medians, but the spreads, 30.3 and 97.5 ms, exceed the difference) and 1.82 against 1.89 ms at 2^12 (inside the spreads: a
 * tie).  The Encodings of the two paths were equal in every case.  Kernel against kernel the lane kernel takes 17.1 / 18.1 / 28.5
 * ms per 2^20 sums of the three shapes (profiles/msm_mixed_kernel_trace.txt), where the variable-base kernel alone takes 14.4 ms
 * per 2^20 [k]P: at (1, 1) the Straus half on 192-byte table entries does not beat the leaner signed-limb chain, and the gain
 * is the three calls and the Element records that no longer cross the bus.
 * Arguments are checked in this order, all on the host before any copy or launch: v, t (D377_ERR_ARG, the message names the
 * argument and the call that serves 0 of them), null buffers when n > 0 (the message names the buffer), ctx, the handle, then
 * the whole n x t index array (the message names base_index and the first offending position); on a refused call no output
 * byte is written; n == 0 with good arguments is D377_OK.  Scratch: the small sums' table scratch for v terms, grown on
 * demand and kept.  A multi-GPU context slices the SUMS over its devices.  These are the host-pointer forms; device buffers take
 * d377_batch_msm_mixed[_encoded]_resident (decaf377_amd_resident.h), which answer the indices with a verdict record. */
#define D377_BATCH_MSM_MIXED_MAX_VAR 8      /* = D377_BATCH_MSM_MAX_TERMS */
int d377_batch_msm_mixed(d377_ctx* ctx, int64_t handle, const int* base_index, const uint8_t* fixed_scalar32, size_t t,
                         const uint64_t* xyzt, const uint8_t* var_scalar32, size_t v, size_t n, uint8_t* enc32_out,
                         uint64_t* xyzt_out);
int d377_batch_msm_mixed_encoded(d377_ctx* ctx, int64_t handle, const int* base_index, const uint8_t* fixed_scalar32, size_t t,
                                 const uint8_t* enc32, const uint8_t* var_scalar32, size_t v, size_t n, uint8_t* enc32_out,
                                 uint64_t* xyzt_out, uint8_t* status);

/* The fixed-base, indexed and mixed sums above also have forms on DEVICE buffers, the resident forms
 * (d377_batch_fixed_msm_resident, d377_batch_fixed_long_msm_resident, d377_batch_fixed_msm_indexed_resident,
 * d377_batch_msm_mixed[_encoded]_resident, d377_check_base_index_resident): they are declared in decaf377_amd_resident.h,
 * which this header includes at its end. */

/* Fq field operations on in-memory elements (4 Montgomery u64 limbs, R = 2^256, fully reduced), the
 * unit everything above is built from             src/fields/fq/u64/wrapper.rs:99-132, fq/ops.rs
 * op: D377_FQ_ADD / SUB / MUL (binary, b != NULL) and D377_FQ_SQUARE / NEG / INVERSE (unary, b NULL).
 * INVERSE mirrors `Fq::inverse() -> Option<Fq>`: status[i] = 1 and a zero record for a zero input
 * (status may be NULL for the other ops).  d377_batch_fq_from_bytes_checked mirrors
 * Fq::from_bytes_checked (src/fields/fq.rs:108-115): status 1 for non-canonical strings. */
#define D377_FQ_ADD 0
#define D377_FQ_SUB 1
#define D377_FQ_MUL 2
#define D377_FQ_SQUARE 3
#define D377_FQ_NEG 4
#define D377_FQ_INVERSE 5
int d377_batch_fq_op(d377_ctx* ctx, int op, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out,
                     uint8_t* status);
int d377_batch_fq_from_bytes_checked(d377_ctx* ctx, const uint8_t* bytes32, size_t n, uint64_t* out, uint8_t* status);
int d377_batch_fq_to_bytes(d377_ctx* ctx, const uint64_t* a, size_t n, uint8_t* bytes32);

/* Fr byte handling (the only part of Fr the hot path uses)            src/fields/fr.rs:82-107
 * from_le_bytes_mod_order: 32 raw bytes -> canonical 32-byte scalar (value mod r);
 * from_bytes_checked: status 1 for strings >= r (the record is copied through when canonical). */
int d377_batch_fr_from_le_bytes_mod_order(d377_ctx* ctx, const uint8_t* bytes32, size_t n, uint8_t* fr32_out);
int d377_batch_fr_from_bytes_checked(d377_ctx* ctx, const uint8_t* bytes32, size_t n, uint8_t* fr32_out, uint8_t* status);

/* Fr arithmetic                                                   src/fields/fr/u64/wrapper.rs:76-108
 * Scalars travel as 32-byte little-endian strings (Fr::to_bytes_le, wrapper.rs:63-70), as in the scalar
 * multiplications above: inputs are any 32 bytes (reduced mod r first), outputs canonical.  op: the D377_FQ_*
 * selectors (ADD / SUB / MUL binary, b32 != NULL; SQUARE / NEG / INVERSE unary, b32 NULL).  INVERSE mirrors
 * `Fr::inverse() -> Option<Fr>`: status[i] = 1 and a zero record for a zero input (status may be NULL for the
 * other ops).  d377_batch_fr_from_wide_bytes: Fr::from_le_bytes_mod_order on 48- or 64-byte strings (hash
 * outputs, `Fr::rand`)                                           src/fields/fr.rs:82-94, 118-126 */
int d377_batch_fr_op(d377_ctx* ctx, int op, const uint8_t* a32, const uint8_t* b32, size_t n, uint8_t* out32,
                     uint8_t* status);
int d377_batch_fr_from_wide_bytes(d377_ctx* ctx, const uint8_t* bytes, size_t len, size_t n, uint8_t* fr32_out);

/* -Element (x, t negated), Element::is_identity (x == 0), and the constants Element::IDENTITY /
 * Element::GENERATOR as one 16 x u64 record each      src/min_curve/element.rs:324-332, 113-117, 53-81 */
int d377_batch_neg(d377_ctx* ctx, const uint64_t* p_xyzt, size_t n, uint64_t* out_xyzt);
int d377_batch_is_identity(d377_ctx* ctx, const uint64_t* p_xyzt, size_t n, uint8_t* is_identity);
void d377_identity(uint64_t xyzt[16]);
void d377_generator(uint64_t xyzt[16]);

/* Device-pointer forms (same semantics). */
int d377_batch_sqrt_ratio_zeta_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* num32,
                                   const uint8_t* den32, size_t n, uint8_t* root32, uint8_t* was_square);
int d377_batch_sqrt_ratio_zeta_ex_dev(d377_ctx* ctx, int dev, void* stream, int root, const uint8_t* num32,
                                      const uint8_t* den32, size_t n, uint8_t* root32, uint8_t* was_square);
int d377_batch_decompress_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, size_t n,
                              uint64_t* xyzt, uint8_t* status);
int d377_batch_compress_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, size_t n,
                            uint8_t* enc32);
int d377_batch_roundtrip_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, size_t n,
                             uint8_t* enc32_out, uint8_t* status);
int d377_batch_scalar_mul_base_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* scalar32,
                                   size_t n, uint8_t* enc32_out);
int d377_batch_scalar_mul_var_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32,
                                  const uint8_t* scalar32, size_t n, uint8_t* enc32_out, uint8_t* status);
int d377_batch_encode_to_curve_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* fq32, size_t n,
                                   uint8_t* enc32_out);
int d377_batch_hash_to_curve_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* r1_32,
                                 const uint8_t* r2_32, size_t n, uint8_t* enc32_out);

int d377_batch_add_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* p_xyzt, const uint64_t* q_xyzt,
                       size_t n, uint64_t* out_xyzt);
int d377_batch_sub_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* p_xyzt, const uint64_t* q_xyzt,
                       size_t n, uint64_t* out_xyzt);
int d377_batch_double_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* p_xyzt, size_t n,
                          uint64_t* out_xyzt);
int d377_batch_eq_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* p_xyzt, const uint64_t* q_xyzt,
                      size_t n, uint8_t* equal);

int d377_batch_fq_op_dev(d377_ctx* ctx, int dev, void* stream, int op, const uint64_t* a, const uint64_t* b, size_t n,
                         uint64_t* out, uint8_t* status);
int d377_batch_neg_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* p_xyzt, size_t n, uint64_t* out_xyzt);
int d377_batch_is_identity_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* p_xyzt, size_t n,
                               uint8_t* is_identity);
int d377_batch_fq_from_wide_bytes_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* bytes, size_t len,
                                      size_t n, uint8_t* fq32_out);
int d377_batch_encode_to_curve_wide_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* bytes, size_t len,
                                        size_t n, uint8_t* enc32_out);
int d377_batch_to_affine_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, size_t n, uint64_t* xy);
int d377_batch_scalar_mul_var_element_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* p_xyzt,
                                          const uint8_t* scalar32, size_t n, uint64_t* out_xyzt);
int d377_batch_scalar_mul_base_element_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* scalar32, size_t n,
                                           uint64_t* out_xyzt);
int d377_batch_compress_to_field_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* p_xyzt, size_t n,
                                     uint64_t* fq_out);
int d377_batch_encode_to_curve_element_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* fq32, size_t n,
                                           uint64_t* out_xyzt);
int d377_batch_hash_to_curve_element_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* r1_32,
                                         const uint8_t* r2_32, size_t n, uint64_t* out_xyzt);
int d377_batch_fq_from_bytes_checked_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* bytes32, size_t n,
                                         uint64_t* out, uint8_t* status);
int d377_batch_fq_to_bytes_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* a, size_t n, uint8_t* bytes32);
int d377_batch_fr_from_le_bytes_mod_order_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* bytes32, size_t n,
                                              uint8_t* fr32_out);
int d377_batch_fr_from_bytes_checked_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* bytes32, size_t n,
                                         uint8_t* fr32_out, uint8_t* status);
int d377_batch_fr_op_dev(d377_ctx* ctx, int dev, void* stream, int op, const uint8_t* a32, const uint8_t* b32, size_t n,
                         uint8_t* out32, uint8_t* status);
int d377_batch_fr_from_wide_bytes_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* bytes, size_t len,
                                      size_t n, uint8_t* fr32_out);
/* MSM on device buffers (the workspace grows inside the context on first use of a larger n). */
int d377_msm_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalar32, size_t n,
                 uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_msm_encoded_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalar32,
                         size_t n, uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status);
int d377_batch_msm_small_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, const uint8_t* scalar32, size_t m,
                             size_t n, uint8_t* enc32_out, uint64_t* xyzt_out);
int d377_batch_msm_small_encoded_dev(d377_ctx* ctx, int dev, void* stream, const uint8_t* enc32, const uint8_t* scalar32,
                                     size_t m, size_t n, uint8_t* enc32_out, uint64_t* xyzt_out, uint8_t* status);
/* Sum of m Element records (e.g. the per-rank partial sums of a sharded MSM after an all-gather). */
int d377_sum_elements_dev(d377_ctx* ctx, int dev, void* stream, const uint64_t* xyzt, size_t m,
                          uint8_t* enc32_out, uint64_t* xyzt_out);


/* Multi-GPU for a batch that already lives in HBM (contiguous slices, scatter of inputs and
 * gather of outputs only, no other exchange).  in0/in1/out0/out1 are the buffers the matching
 * d377_batch_*_dev entry point takes, in its order (unused ones NULL), resident on device `root_dev` of
 * the context; slice k of the batch runs on device k (peer copies over xGMI for k != root_dev, in place
 * for the root), and `stream` (a stream of the root device) continues once every slice is back. */
#define D377_OP_SQRT_RATIO_ZETA 0
#define D377_OP_DECOMPRESS 1
#define D377_OP_COMPRESS 2
#define D377_OP_ROUNDTRIP 3
#define D377_OP_SCALAR_MUL_BASE 4
#define D377_OP_SCALAR_MUL_VAR 5
#define D377_OP_ENCODE_TO_CURVE 6
#define D377_OP_HASH_TO_CURVE 7
#define D377_OP_SCALAR_MUL_VAR_ELEMENT 8
#define D377_OP_SCALAR_MUL_BASE_ELEMENT 9
int d377_batch_sharded_dev(d377_ctx* ctx, int root_dev, void* stream, int op, const void* in0, const void* in1, size_t n,
                           void* out0, void* out1);

#ifdef __cplusplus
}
#endif

#include "decaf377_amd_resident.h"
#include "decaf377_amd_long_sums.h"
#include "decaf377_amd_bucket_sums.h"
#include "decaf377_amd_ragged_sums.h"
#include "decaf377_amd_segmented_sums.h"
#include "decaf377_amd_short_msm.h"

#endif /* DECAF377_AMD_H */
