"""k_scalar_mul_var / k_scalar_mul_var_el on the GPU with the lean chain (curve.hpp ge_scalar_mul_w4_lean: 62 windows from
a start value lifted from table entry d62, doublings that take 2XY from a squaring).  Both calls are forced onto the lane
kernels with the small_max tuning key, as tests/test_vb_packed_table_gpu.py does; every output byte and status is compared
against the oracle.  Sizes: a single element, a partial wave (63), one past a wave (65), one past a workgroup (257), one past a
chunk of 8 x 256 elements (2049) and one past two chunks (4097), so that a lane set is claimed a second time.  The special
scalars (each top window digit 0..5, the digit 8 and its carry at several windows, 0, 1, 2, r - 1, r - 2, 2^256 - 1) and the
special points (identity, non-canonical, negative s, off the curve) sit at the start, in the second chunk and at the end.
Needs a real MI355X: `-m gpu`."""
import numpy as np
import pytest

from _vb_lean_cases import le as _le, special_points, special_scalars

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 65, 257, 2049, 4097)
N_MAX = max(SIZES)


@pytest.fixture(scope="module")
def ctx():
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)                    # no fixed-base leg here: the comb is not built
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(oracle):
    """N_MAX (encoding, scalar) pairs and the oracle's answers, computed once; every size takes a prefix"""
    rng = np.random.default_rng(9377)
    n = N_MAX
    valid = oracle.encode_to_curve(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    enc = valid.copy()
    k = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sp = special_scalars()
    pts = special_points(oracle, valid)
    m = len(sp)
    assert 2 * m < 63 and 2048 + 2 * m < n - 2 * m
    for base in (0, 2048, n - 2 * m):                      # the start (n = 1: the scalar 0), the second chunk, the end
        for j, v in enumerate(sp):
            k[base + 2 * j] = _le(v)                       # on a valid point
            k[base + 2 * j + 1] = _le(sp[-1 - j])          # on a special point
            enc[base + 2 * j + 1] = pts[j % 4]
    out, st = oracle.scalar_mul_var(enc, k)
    assert st[0] == 0 and st[1] == 0 and st[3] != 0 and st[5] != 0 and st[7] != 0 and 0 < st.mean() < 0.1
    xyzt, st_d = oracle.decompress(valid)
    assert not st_d.any()
    el_in = oracle.scalar_mul_xyzt(xyzt, rng.integers(0, 256, (n, 32), dtype=np.uint8))     # Elements with Z != 1
    el = oracle.compress(oracle.scalar_mul_xyzt(el_in, k))
    return {"enc": enc, "k": k, "out": out, "st": st, "el_in": el_in, "el": el}


@pytest.mark.parametrize("n", SIZES)
def test_lean_chain_lane_route_matches_oracle(ctx, case, n):
    with ctx.tuning(small_max=0):                          # one lane per element, whatever the size
        out, st = ctx.scalar_mul_var(case["enc"][:n], case["k"][:n])
        el = ctx.compress(ctx.scalar_mul_var_element(case["el_in"][:n], case["k"][:n]))
    assert (st == case["st"][:n]).all(), n
    assert (out == case["out"][:n]).all(), n
    assert not out[st != 0].any()                          # a rejected encoding leaves an all-zero output
    assert (el == case["el"][:n]).all(), n
    assert ctx.health()[0] == 0
