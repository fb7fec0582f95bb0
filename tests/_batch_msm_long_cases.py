"""The cases that tests/test_batch_msm_long_host.py and tests/test_batch_msm_long_gpu.py share: the plan as the issue of
d377_batch_msm_long states it (restated here, independent of batch_msm_long_plan.hpp), the builder of the planted cases,
and the oracle's fold of scalar multiplications and additions."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from _sums_support import R, scalar_bytes as _scalar_bytes

THREADS = 16


def plan(m):
    """(g, b) as the issue states them: g = ceil(m / 8) groups, b = ceil(m / g) terms per group."""
    g = -(-m // 8)
    return g, -(-m // g)


def make_case(oracle, rng, n, m, encoded=False):
    """n sums of m > 8 terms with the planted cases -> (points, scalars, what is planted where).  points: [n m, 16] Elements,
    or [n m, 32] Encodings with invalid ones (bit 0x40 of byte 31) where an Element case has a Z = 0 record, on every 9th
    term and on the last term of sum 0.
      sum 0              scalars 0, 1, r - 1, r, 2^256 - 1 on terms 0 .. 4, a dead record on term 5, one point on terms 6 and 7
      sum 1 (0 if n = 1) k P in the first group that is free and (r - k) P on the last term, in different groups; with a sum of
                         its own every other scalar is 0: the identity
      sum 2 (0 if n < 3) one group whose terms are all dead (the last group where it has a sum of its own, else group 2)
      sum 3 (if n > 3)   every term dead
      sum 4 (if n > 4)   group 0 all dead"""
    g, b = plan(m)
    pts = oracle.elligator_map_xyzt(rng.integers(0, 256, (n * m, 32), dtype=np.uint8))
    k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
    dead = np.zeros(n * m, bool)
    for j, v in enumerate([0, 1, R - 1, R, (1 << 256) - 1]):
        k[j] = _scalar_bytes(v)
    dead[5] = True
    pts[7] = pts[6]
    info = {"identity": []}
    kv = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % R
    if n >= 2:
        lo = m
        k[lo:lo + m] = 0
        a = lo
        info["identity"].append(1)
    else:
        a = 8                                                    # group 1 (b = 8 at the m this is used with)
    z = a - a % m + m - 1                                        # the last term of the same sum: the last group
    pts[z] = pts[a]
    k[a], k[z] = _scalar_bytes(kv), _scalar_bytes(R - kv)
    assert (a % m) // b != (z % m) // b
    if n >= 3:
        dead[2 * m + (g - 1) * b:3 * m] = True
    else:
        assert g > 3 and b == 8
        dead[2 * b:3 * b] = True
    if n > 3:
        dead[3 * m:4 * m] = True
        info["identity"].append(3)
    if n > 4:
        dead[4 * m:4 * m + b] = True
    if encoded:
        dead[8::9] = True
        dead[m - 1] = True
        enc = oracle.compress(pts)
        enc[dead, 31] |= 0x40
        info["dead"] = dead
        return enc, k, info
    rec = pts.reshape(n * m, 4, 4)
    rec[dead, 2] = 0                                             # Z = 0: no group element, counts as the identity
    info["dead"] = dead
    return np.ascontiguousarray(rec.reshape(n * m, 16)), k, info


def oracle_fold(oracle, points, k, m):
    """The oracle's sums: scalar multiplications (on THREADS threads) and a tree of additions per sum; a dead term -- an
    invalid Encoding, a record with Z = 0 -- is 0 * identity -> (encodings [n, 32], records [n, 16], status per term or None)."""
    terms = points.shape[0]
    n = terms // m
    status = None
    if points.shape[1] == 32:
        pts, status = oracle.decompress(points)
        dead = status != 0
    else:
        pts = np.ascontiguousarray(points, dtype=np.uint64)
        dead = ~pts.reshape(terms, 4, 4)[:, 2].any(axis=1)
    pts = np.where(dead[:, None], oracle.identity_xyzt()[None, :], pts).astype(np.uint64)
    kk = np.where(dead[:, None], 0, k).astype(np.uint8)
    bounds = np.linspace(0, terms, THREADS + 1).astype(int)
    with ThreadPoolExecutor(THREADS) as ex:
        parts = list(ex.map(lambda t: oracle.scalar_mul_xyzt(np.ascontiguousarray(pts[bounds[t]:bounds[t + 1]]),
                                                             np.ascontiguousarray(kk[bounds[t]:bounds[t + 1]])), range(THREADS)))
    acc = np.concatenate(parts).reshape(n, m, 16)
    while acc.shape[1] > 1:                                      # halve the term axis
        c = acc.shape[1]
        h = c // 2
        s = oracle.add_xyzt(np.ascontiguousarray(acc[:, :h]).reshape(-1, 16), np.ascontiguousarray(acc[:, h:2 * h]).reshape(-1, 16)).reshape(n, h, 16)
        acc = np.concatenate([s, acc[:, 2 * h:]], axis=1) if c % 2 else s
    acc = np.ascontiguousarray(acc[:, 0])
    return oracle.compress(acc), acc, status
