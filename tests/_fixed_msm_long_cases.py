"""What tests/test_fixed_msm_long_host.py and tests/test_fixed_msm_long_gpu.py share: the cut of
decaf377_amd/csrc/fixed_msm_long_plan.hpp restated in Python, bases and scalars with the degenerate ones at the first position of
a segment (the record the walk lifts with ge_from_cached_affine), and the oracle's sums two ways -- scalar multiplications and
additions, and the byte-table fold of tests/_sums_support.py for batches too large for the first."""
import numpy as np

from _sums_support import R, scalar_bytes

SPECIAL = [0, 1, R - 1, R, (1 << 256) - 1]
KINDS = ["identity", "generator", "scaled", "torsion"]
FOLD = 16


def plan(m, n, L, seg_min=1):
    """(g, b): segments per sum and bases per segment for n sums over m bases on L resident lanes."""
    if n >= L:
        return 1, m
    cap, most = -(-L // n), -(-m // seg_min)
    g0 = min(most, cap)
    b = -(-m // g0)
    g = -(-m // b)
    if n * g + n < min(L, n * most):                             # rounding b up lost more than a segment per sum: round it down
        b -= 1
        g = -(-m // b)
    return g, b


def levels(g):
    n = 0
    while g > 1:
        g = -(-g // FOLD)
        n += 1
    return n


def make_bases(oracle, rng, m, b):
    """m bases, random Elligator outputs except at the segment-first positions q b, which cycle through the identity,
    GENERATOR, a representative with Z != 1 and one that differs from its point by the 2-torsion point (0, -1)."""
    pts = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (m, 32), dtype=np.uint8)), dtype=np.uint64)
    for q, j in enumerate(range(0, m, b)):
        if q >= 2 * len(KINDS):
            break
        kind = KINDS[(q + m) % len(KINDS)]
        if kind == "identity":
            pts[j] = oracle.identity_xyzt()
        elif kind == "generator":
            pts[j] = oracle.generator_xyzt()
        elif kind == "scaled":                                      # (lX, lY, lZ, lT): the same point, Z != 1
            lam = np.tile(oracle.elligator_map_xyzt(rng.integers(0, 256, (1, 32), dtype=np.uint8))[0][:4], (4, 1))
            pts[j] = oracle.fq_op(2, pts[j].reshape(4, 4), lam)[0].reshape(16)
        else:                                                      # (-X, -Y, Z, T) = P + (0, -1)
            p = pts[j].reshape(4, 4).copy()
            p[:2] = oracle.fq_op(4, p[:2])[0]
            pts[j] = p.reshape(16)
    return pts


def make_scalars(rng, n, m, g, b):
    """n x m random scalars, term-major; 0, 1, r - 1, r and 2^256 - 1 each at the first position of a segment of one of the
    sums 0 .. n-2 (no two in the same place), and every scalar of the last sum 0.  n >= 2, and (n - 1) g >= 5."""
    assert n >= 2 and (n - 1) * g >= len(SPECIAL)
    k = rng.integers(0, 256, (n, m, 32), dtype=np.uint8)
    for t, v in enumerate(SPECIAL):
        s, q = t % (n - 1), (t // (n - 1)) % g
        k[s, q * b] = scalar_bytes(v)
    k[n - 1] = 0
    return np.ascontiguousarray(k.reshape(n * m, 32))


def oracle_fold(oracle, bases, k, n, m):
    """sum_j k[i m + j] * B_j by the oracle's scalar multiplications and additions -> (encodings, records)."""
    terms = oracle.scalar_mul_xyzt(np.ascontiguousarray(np.tile(bases, (n, 1))), k).reshape(n, m, 16)
    acc = np.ascontiguousarray(terms[:, 0])
    for j in range(1, m):
        acc = oracle.add_xyzt(acc, np.ascontiguousarray(terms[:, j]))
    return oracle.compress(acc), acc
