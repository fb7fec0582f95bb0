// msm_long_fold.hpp -- what fixed_bases.hip sees of batch_msm_long.hip: the per-device partials area, the fold of g partial
// sums per sum (k_msm_long_fold) and the chunked compressor pass over the folded records.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "host_state.hpp"

namespace d377 {
// The partials area of device `d`, large enough for n sums of g partial sums each and the records of their fold levels; the
// n g partial sums go to its start, sum-major (record s g + q).  The area may not grow inside a stream capture (D377_ERR_ARG).
// The caller holds ctx->mu and the scope of the lane-set guard (GuardScope on d.vb_guard), not yet acquired.
int long_sums_partials(DeviceState& d, hipStream_t s, size_t n, size_t g, uint64_t** partials);
// The same area sized by its caller (batch_msm_segmented.hip: the slot spaces of its levels, its compact records and, behind
// them, the offsets a host form uploads): room for `records` records and `tail_bytes` more.  The same rules.
int long_sums_partials_records(DeviceState& d, hipStream_t s, size_t records, size_t tail_bytes, uint64_t** partials);
// Folds the n x g partial sums at the start of the partials area (g > 1) until one record per sum is left -- the last level
// writes into xyzt_out when that is not null -- and compresses the n sums into out32 in chunks with batched inversions
// (codec_chunked.hip; the caller has asked codec_chunked_ok).  Enqueued on `s`; the caller holds the acquired guard scope.
int long_sums_fold_compress(DeviceState& d, hipStream_t s, size_t n, size_t g, uint8_t* out32, uint64_t* xyzt_out);
}  // namespace d377
