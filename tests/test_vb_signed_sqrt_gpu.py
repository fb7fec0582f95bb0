"""k_scalar_mul_var / k_scalar_mul_var_el on the GPU after two changes of their lane code: the decompression's square root
runs on signed limbs (curve.hpp: ge_decompress<fes>), and the window table's entry 0 is one shared identity record that no
lane stores (d377.hip GlobalTab).  Every output byte and status against the oracle, on the one-lane-per-element route
(forced with the small_max tuning key, as the route tests do) at sizes with partial waves, a partial workgroup, several
chunks, and lanes that reuse their table for a second element.  Needs a real MI355X: run with `-m gpu`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q = 725501752471715841 | 6461107452199829505 << 64 | 6968279316240510977 << 128 | 1345280370688173398 << 192
R_ORDER = 2111115437357092606062206234695386632838870926408408195193685246394721360383
N_MAX = 2 * 256 * 3 + 5
SIZES = (1, 63, 64, 65, 257, N_MAX)


def _le(v):
    return np.frombuffer(int(v % (1 << 256)).to_bytes(32, "little"), np.uint8)


def _special_scalars():
    h8 = 16 ** 62 - 8 * (16 ** 62 - 1) // 15              # window digits: 1, then -8 sixty-two times
    return [0, 1, R_ORDER - 1, R_ORDER, (1 << 256) - 1,
            2 * R_ORDER,                                   # k / 2 mod r = 0: every window of the recoding zero
            (2 * h8) % R_ORDER, h8,                        # all -8: for the kernel that halves (k = 2h) and the one that does not
            (2 * (7 * (16 ** 62 - 1) // 15)) % R_ORDER, 2, R_ORDER + 1]


@pytest.fixture(scope="module")
def ctx():
    import decaf377_amd as d
    c = d.Context([0], comb_lazy=True)                    # no fixed-base leg here: the comb is not built
    yield c
    c.close()


@pytest.fixture(scope="module")
def case(oracle):
    """N_MAX (encoding, scalar) pairs and the oracle's answers, computed once; every size takes a prefix.  The encodings
    cycle through: valid, valid, the identity, and one of decompression's rejection rules (negative s, s + q, each of the
    top three bits set, an even field element off the curve, values around q and 2^253) -- so valid and rejected lanes
    alternate inside every wave, from the first element on."""
    rng = np.random.default_rng(9377)
    n = N_MAX
    valid = oracle.encode_to_curve(rng.integers(0, 256, (n, 32), dtype=np.uint8))
    ints = [int.from_bytes(bytes(x), "little") for x in valid]
    even = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    even[:, 0] &= 0xFE
    even[:, 31] &= 0x0F
    around = [Q - 2, Q - 1, Q, Q + 1, Q + 2, (1 << 253) - 2, 1 << 253, (1 << 256) - 2, 2, 4, 6]
    enc = valid.copy()
    for i in range(n):
        if i % 4 == 2:
            enc[i] = 0
        elif i % 4 == 3:
            rule = (i // 4) % 7
            if rule == 0:
                enc[i] = _le((Q - ints[i]) % Q)
            elif rule == 1:
                enc[i] = _le(ints[i] + Q)
            elif rule in (2, 3, 4):
                enc[i, 31] |= np.uint8(1 << (rule + 3))
            elif rule == 5:
                enc[i] = even[i]
            else:
                enc[i] = _le(around[(i // 28) % len(around)])
    k = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sp = _special_scalars()
    for j, v in enumerate(sp):                             # on valid points from element 0 on (n = 1: the scalar 0), ...
        k[4 * j] = _le(v)
        k[4 * j + 2] = _le(sp[-1 - j])                     # ... on the identity, ...
        k[n - 1 - j] = _le(v)                              # ... and in the last, partial chunk
        k[520 + j] = _le(v)                                # ... and as a lane's second element (chunks of 2 x 256)
    out, st = oracle.scalar_mul_var(enc, k)
    assert 0.1 < st.mean() < 0.4 and st[0] == 0 and st[2] == 0 and not out[0].any()
    xyzt, st_d = oracle.decompress(valid)
    assert not st_d.any()
    el = oracle.compress(oracle.scalar_mul_xyzt(xyzt, k))
    return {"enc": enc, "k": k, "out": out, "st": st, "valid_xyzt": xyzt, "el": el}


def _check(ctx, case, n, **tuning):
    with ctx.tuning(small_max=0, **tuning):                # one lane per element, whatever the size
        out, st = ctx.scalar_mul_var(case["enc"][:n], case["k"][:n])
        el = ctx.compress(ctx.scalar_mul_var_element(case["valid_xyzt"][:n], case["k"][:n]))
    assert (st == case["st"][:n]).all(), (n, tuning)
    assert (out == case["out"][:n]).all(), (n, tuning)
    assert not out[st == 1].any()
    assert (el == case["el"][:n]).all(), (n, tuning)


@pytest.mark.parametrize("n", SIZES)
def test_lane_route_matches_oracle(ctx, case, n):
    """Partial waves (1, 63, 65), a full one, a partial workgroup (257) and 2 * 256 * 3 + 5: every output byte and status
    of scalar_mul_var, and the group elements of scalar_mul_var_element, equal the oracle's."""
    _check(ctx, case, n)
    assert ctx.health()[0] == 0


@pytest.mark.parametrize("per_lane", (1, 2, 3))
def test_table_reused_by_a_lane(ctx, case, per_lane):
    """Chunks of per_lane x 256 elements: at 2 and 3 a lane runs several elements over the same table with no identity
    rewritten in between; 2 * 256 * 3 + 5 elements are three full chunks of two per lane and a partial one, and with one
    per lane more chunks than a small grid has workgroups' worth of rounds."""
    _check(ctx, case, N_MAX, chunk_per_lane=per_lane)
    _check(ctx, case, 2 * 256 + 1, chunk_per_lane=per_lane)      # a lane with 2 elements next to lanes with 1 (per_lane >= 2)
    assert ctx.health()[0] == 0


def test_stale_scratch_does_not_matter(ctx, case, oracle):
    """Another operation that works in the lanes' table scratch first (msm_small, a lane per sum), then the call under test
    again: whatever the tables' slots 0 hold, the results are the oracle's."""
    n = N_MAX
    rng = np.random.default_rng(11)
    m_enc = oracle.encode_to_curve(rng.integers(0, 256, (5000, 32), dtype=np.uint8))
    m_k = rng.integers(0, 256, (5000, 32), dtype=np.uint8)
    _check(ctx, case, n)
    sums, m_st = ctx.msm_small(m_enc, m_k, 2)              # 2 500 two-term sums: the lane-per-sum kernel
    assert not np.asarray(m_st).any()
    terms = oracle.scalar_mul_xyzt(oracle.decompress(m_enc[:64])[0], m_k[:64]).reshape(32, 2, 16)
    want = oracle.compress(oracle.add_xyzt(np.ascontiguousarray(terms[:, 0]), np.ascontiguousarray(terms[:, 1])))
    assert (np.asarray(sums)[:32] == want).all()
    with ctx.tuning(small_max=0):                          # other points through the same tables, then the case again
        ctx.scalar_mul_var(case["enc"][::-1][:n].copy(), case["k"][:n])
    _check(ctx, case, n)
    _check(ctx, case, 65)
    assert ctx.health()[0] == 0                            # no lane set left claimed
