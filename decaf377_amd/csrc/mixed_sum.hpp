// mixed_sum.hpp -- the per-sum body of the mixed sums (batch_msm_mixed.hip):
//     sum_{j < t} f_j B_{index_j}  +  sum_{p < v} k_p P_p
// with the B registered as combs (fixed_bases.hip) and the P variable points.  Both existing walks run on halved scalars:
// straus_sum (straus.hpp) yields Hv = sum (k_p / 2) P_p, ge_fixed_msm_indexed_w8 (curve.hpp) yields Hf = sum (f_j / 2) B.  One
// unified addition joins them, H = Hv + Hf, and the sum is 2 H: its Encoding comes out of the square-root-free compressor
// (ge_dcb_from_half), the caller's, as for either walk alone.  Plain per-lane arithmetic, shared by the device kernel and the
// host simulation (tests/host_sim/msm_mixed_sim.cpp), whose bounds build walks it.
//
// Bounds of the join.  Every coordinate of Hv is the result of a product: v >= 1, so the chain's last step is a
// ge_add_cached_reload, whose X, Y, Z are fe_mul results and whose T is one because want_t asks for it.  Every coordinate of
// Hf is one as well: a comb has at least two windows, so the walk ends in a ge_add_affine with T requested.  A product's result
// has carried limbs and a value below 2q.  ge_add forms y - x and y + x of each operand, the sum or offset difference of two such
// values -- the operands the same function meets when partial sums are folded (msm_long_fold.hpp) and when the comb builder adds
// a base to an accumulator -- multiplies them pairwise, and forms 2 z1 and K t1 t2 from products again; nothing in it depends on
// which walk an operand came from.  The -DD377_BOUNDS build of the host simulation asserts every one of these preconditions
// on every case of tests/test_msm_mixed_host.py, the doubling and the cancelling join among them.
#pragma once
#include <stdint.h>

#include "curve.hpp"
#include "straus.hpp"

namespace d377 {

// [1/2] of the mixed sum.  st / v / load_var_scalar / load_point: straus_sum's arguments.  t / tload / ftab: those of
// ge_fixed_msm_indexed_w8, tload(j, k) -> comb with the scalar left reduced, halved and masked.  T of the result is always
// computed (the join is a full addition): callers that store the Element read it, the compressor does not.
template <int BITS, class Tab, class LoadScalar, class LoadPoint, class TLoad, class FTab>
D377_HD ge mixed_half_sum(Tab& st, int v, LoadScalar load_var_scalar, LoadPoint load_point, int t, TLoad&& tload, const FTab& ftab) {
  const ge hv = straus_sum(st, v, load_var_scalar, load_point, /*want_t=*/true);
  const ge hf = ge_fixed_msm_indexed_w8<BITS>(t, tload, ftab, /*want_t=*/true);
  return ge_add(hv, hf);
}

}  // namespace d377
