// index_verdict.hpp -- the verdict on an array of base indices (fixed_bases.hip: k_index_verdict): which entries of
// `base_index` the indexed and mixed sums refuse, and how the verdicts of two parts of an array combine.  A resident call
// cannot read its indices on the host without a synchronisation, so it has the device write ONE record per call:
//     verdict[0]   how many entries are neither -1 nor a base 0 .. m-1
//     verdict[1]   the position of the first such entry, or INDEX_VERDICT_NONE where there is none
// Plain integer code shared by the kernel and a host program (tests/cpp/index_verdict.cpp), which checks it against numpy
// (tests/test_resident_sums_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fq29.hpp"

namespace d377 {

constexpr uint64_t INDEX_VERDICT_NONE = ~(uint64_t)0;

struct IndexVerdict {
  uint64_t count, first;
};

// -1 is an absent term; the sums kernels' unsigned compare treats every other index outside 0 .. m-1 as absent too, and
// this is the predicate that counts those
D377_HD bool index_refused(int b, int m) { return b != -1 && (uint32_t)b >= (uint32_t)m; }

D377_HD IndexVerdict verdict_none() { return IndexVerdict{0, INDEX_VERDICT_NONE}; }
D377_HD IndexVerdict verdict_of(int b, int m, uint64_t position) {
  return index_refused(b, m) ? IndexVerdict{1, position} : verdict_none();
}
// the verdict on two parts of an array from the verdicts on each: associative and commutative, verdict_none() its unit
D377_HD IndexVerdict verdict_join(const IndexVerdict& a, const IndexVerdict& b) {
  return IndexVerdict{a.count + b.count, a.first < b.first ? a.first : b.first};
}

}  // namespace d377
