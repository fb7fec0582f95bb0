// comb_tabs.hpp -- how the sums over registered bases read a handle's combs and pick the kernels of its width
// (fixed_bases.hip, batch_msm_mixed.hip and no other unit).  Not part of fixed_comb.hpp: d377.hip includes that one, and its
// kernels' code generation is guarded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "curve.hpp"
#include "device_util.hpp"
#include "host_state.hpp"

namespace d377 {

// the m combs of a handle, back to back: entry c of window i of base j
template <int BITS>
struct CombTabs {
  const uint32_t* base;
  __device__ __forceinline__ gea load(int j, int i, int c, bool swap) const {
    return pt_load_affine(base + (((size_t)j * FbShape<BITS>::windows + i) * FbShape<BITS>::entries + c) * FBW_ENTRY_WORDS, swap);
  }
};

// The comb widths a handle may ask for, and their index in the per-width caches of DeviceState;
// f(std::integral_constant<int, BITS>) runs with the kernels of that width, any other width is refused with `refusal`.
inline int width_slot(int bits) { return bits == 8 ? 0 : bits == 12 ? 1 : bits == 16 ? 2 : bits == 18 ? 3 : -1; }
template <class F>
int with_width(int bits, const char* refusal, F&& f) {
  switch (bits) {
    case 8: return f(std::integral_constant<int, 8>{});
    case 12: return f(std::integral_constant<int, 12>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 18: return f(std::integral_constant<int, 18>{});
  }
  return fail(D377_ERR_ARG, "%s", refusal);
}

}  // namespace d377
