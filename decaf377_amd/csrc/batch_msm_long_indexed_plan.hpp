// batch_msm_long_indexed_plan.hpp -- what a slot of a chain of d377_batch_long_msm_indexed (batch_msm_long_indexed.hip) is.
// The sums are cut by batch_msm_long_plan.hpp's LongPlan, also for m <= 8 (g = 1, b = m: one chain per sum and no fold level);
// slot p of group q of sum s is term s m + q b + p, and a term names its point: point_index[term] is a record of the pool.
// Plain integer code shared by the kernels and the host simulation (tests/host_sim/batch_msm_long_indexed_sim.cpp).
//
//   SLOT_PAST     past the end of the sum (the last group's padding): no index, no scalar and no point is read
//   SLOT_ABSENT   the index is -1, or it is refused -- any other value outside 0 .. pool_count - 1, which the host form has
//                 turned down before any launch and the resident form's verdict counts (index_verdict.hpp: the same unsigned
//                 compare): no scalar and no point is read, so no index can address past the pool
//   SLOT_LIVE     record point_index[term] of the pool, scalar `term`
// A slot that is not live is DEAD to its chain: the identity with digits 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "batch_msm_long_plan.hpp"

namespace d377 {

enum LongSlotKind { SLOT_PAST = 0, SLOT_ABSENT = 1, SLOT_LIVE = 2 };

struct LongSlot {
  int kind;
  size_t term;                           // the slot's scalar and index (not SLOT_PAST)
  size_t record;                         // the pool record (SLOT_LIVE)
};

// pool_count: 1 .. 2^31 - 1, so -1 (0xffffffff) fails the unsigned compare like every other index outside the pool
D377_BML_HD bool pool_index_live(int index, uint32_t pool_count) { return (uint32_t)index < pool_count; }

D377_BML_HD LongSlot long_indexed_slot(const LongPlan& plan, size_t s, size_t q, int p, const int* point_index, uint32_t pool_count) {
  LongSlot r;
  r.kind = SLOT_PAST; r.term = 0; r.record = 0;
  if ((size_t)p >= plan.count(q)) return r;
  r.term = s * plan.m + plan.first(q) + (size_t)p;
  const int index = point_index[r.term];
  r.kind = SLOT_ABSENT;
  if (!pool_index_live(index, pool_count)) return r;
  r.kind = SLOT_LIVE;
  r.record = (size_t)(uint32_t)index;
  return r;
}

}  // namespace d377
