"""k_scalar_mul_var / k_scalar_mul_var_el on the GPU over the packed window table: an entry is four 256-bit integers in one
128-byte line (d377.hip GlobalTab, fqs29.hpp fes_pack256).  Both calls are forced onto the lane kernels with the small_max
tuning key, as the route tests do; every output byte and status is compared against the oracle.  Sizes: a single element, a
partial wave (63), one past a wave (65), one past a workgroup (257), one past a chunk of 8 x 256 elements (2049) and one past
two chunks (4097), so that a lane set is claimed a second time and its tables are rewritten.  Needs a real MI355X: `-m gpu`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q = 725501752471715841 | 6461107452199829505 << 64 | 6968279316240510977 << 128 | 1345280370688173398 << 192
R_ORDER = 2111115437357092606062206234695386632838870926408408195193685246394721360383
SIZES = (1, 63, 65, 257, 2049, 4097)
N_MAX = max(SIZES)


def _le(v):
    return np.frombuffer(int(v % (1 << 256)).to_bytes(32, "little"), np.uint8)


def _special_scalars():
    # 8 * 16^i: the digit 8 (read as -8 from entry 8) and its carry into the next window; for the kernel that halves the
    # scalar first (k_scalar_mul_var) the doubled values give the same digits
    eights = [8 * 16 ** i for i in (0, 1, 7, 31, 61)]
    return [0, 1, R_ORDER - 1] + eights + [2 * e % R_ORDER for e in eights]


@pytest.fixture(scope="module")
def ctx():
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)                    # no fixed-base leg here: the comb is not built
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(oracle):
    """N_MAX (encoding, scalar) pairs and the oracle's answers, computed once; every size takes a prefix.  Encodings cycle
    through valid, valid, all-zero (the identity) and two invalid ones (not a field element; a negative s)."""
    rng = np.random.default_rng(128377)
    n = N_MAX
    valid = oracle.encode_to_curve(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    ints = [int.from_bytes(bytes(x), "little") for x in valid]
    enc = valid.copy()
    for i in range(n):
        if i % 4 == 2:
            enc[i] = 0
        elif i % 8 == 3:
            enc[i] = 0xFF
        elif i % 8 == 7:
            enc[i] = _le((Q - ints[i]) % Q)
    k = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sp = _special_scalars()
    for j, v in enumerate(sp):
        k[4 * j] = _le(v)                                  # on valid points, from element 0 on (n = 1: the scalar 0)
        k[4 * j + 2] = _le(sp[-1 - j])                     # on the identity
        k[2048 + 4 * j] = _le(v)                           # in the second chunk
        k[n - 1 - 4 * j] = _le(v)                          # at the end (4096: the one element of the third chunk)
    out, st = oracle.scalar_mul_var(enc, k)
    assert 0.1 < st.mean() < 0.4 and st[0] == 0 and st[2] == 0 and st[3] != 0 and st[7] != 0 and not out[0].any()
    xyzt, st_d = oracle.decompress(valid)
    assert not st_d.any()
    el = oracle.compress(oracle.scalar_mul_xyzt(xyzt, k))
    return {"enc": enc, "k": k, "out": out, "st": st, "valid_xyzt": xyzt, "el": el}


@pytest.mark.parametrize("n", SIZES)
def test_packed_table_lane_route_matches_oracle(ctx, case, n):
    with ctx.tuning(small_max=0):                          # one lane per element, whatever the size
        out, st = ctx.scalar_mul_var(case["enc"][:n], case["k"][:n])
        el = ctx.compress(ctx.scalar_mul_var_element(case["valid_xyzt"][:n], case["k"][:n]))
    assert (st == case["st"][:n]).all(), n
    assert (out == case["out"][:n]).all(), n
    assert not out[st != 0].any()                          # a rejected encoding leaves an all-zero output
    assert (el == case["el"][:n]).all(), n
    assert ctx.health()[0] == 0
