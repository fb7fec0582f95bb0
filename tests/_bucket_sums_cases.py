"""The cases that tests/test_bucket_sums_host.py and tests/test_bucket_sums_gpu.py share: the plan of d377_batch_bucket_msm
as its header states it (restated here, independent of msm_batch_plan.hpp), and the builder of the planted cases.  The
oracle's fold is tests/_batch_msm_long_cases.py's, the scalars with chosen digits tests/_digit_cases.py's."""
import numpy as np

import _digit_cases as dc
from _batch_msm_long_cases import oracle_fold  # noqa: F401  (re-exported)
from _sums_support import scalar_bytes as _scalar_bytes

R = dc.R
MAX_TERMS = 1 << 20
# (n, m, window_bits): one term; one pass of three sums; three passes of 4, 4 and 1 sums at the widest window; one pass with
# int32 keys (17 * 2^11 > 2^15); one pass with int16 keys whose magnitude reaches 2^15 (16 * 2^11)
WALK = [(1, 1, 4), (3, 5, 4), (9, 33, 16), (17, 40, 12), (16, 40, 12)]


def windows(c):
    return -(-252 // c)


def window_rule(m):
    """The width in 4 .. 16 that minimises W(c) (m + 9 * 2^(c-1) + 400), the narrower on a tie: the weights fitted to the
    window sweep (profiles/bucket_sums_window_sweep.txt)."""
    return min(range(4, 17), key=lambda c: (windows(c) * (m + (9 << (c - 1)) + 400), c))


def sums_per_pass(n, m, c):
    return max(1, min(n, (1 << 17) >> (c - 1), max(1, (1 << 24) // m)))


def passes(n, m, c):
    """[(first sum, sums)] of every pass."""
    k = sums_per_pass(n, m, c)
    return [(lo, min(k, n - lo)) for lo in range(0, n, k)]


def key(k, c, d):
    if d == 0:
        return 0
    v = (k << (c - 1)) + abs(d)
    return -v if d < 0 else v


def cover_scalars(c):
    """A few of msm_cases(c) -- chosen greedily -- that together reach every claimed (window, digit) pair of the layout: the
    lowest and the highest bucket of every window below the top and the top window's largest digit."""
    layout = dc.msm(c)
    want = dc.claimed_pairs(layout)
    cases = [(h, set(enumerate(d)) & want) for _, d, h in dc.msm_cases(c)]
    chosen = []
    while want:
        h, got = max(cases, key=lambda t: len(t[1] & want))
        assert got & want
        chosen.append(h)
        want -= got
    return chosen


def make_case(oracle, rng, n, m, c, encoded=False, projective=False):
    """n sums of m terms for window width c -> (points, scalars, info).  points: [n m, 16] Elements, or [n m, 32] Encodings
    with invalid ones (bit 0x40 of byte 31) where an Element case has a Z = 0 record.
      the first and the last sum of every pass   the scalars of cover_scalars(c) on their first terms (where m holds them), so
                         that the lowest and the highest bucket of every window of the boundary sums are reached
      the first sum that is no boundary          scalars 0, 1, r - 1, r, 2^256 - 1; a dead record; one point on two terms; k P and
                         (r - k) P -- as many of these, in this order, as m holds
      the second such sum                        every term dead: the all-zero Encoding
      the third                                  k P and (r - k) P with every other scalar 0: the all-zero Encoding
      every 9th term of the call                 dead (unless it carries a cover scalar)
    Element records have Z = 1; projective: those of the last sum keep the Z != 1 of the map to the curve (the shared-inversion
    prepare)."""
    terms = n * m
    mapped = oracle.elligator_map_xyzt(rng.integers(0, 256, (terms, 32), dtype=np.uint8))    # projective records: Z != 1
    pts = np.ascontiguousarray(oracle.decompress(oracle.compress(mapped))[0], dtype=np.uint64)   # the same points with Z = 1
    k = rng.integers(0, 256, (terms, 32), dtype=np.uint8)
    dead = np.zeros(terms, bool)
    keep = np.zeros(terms, bool)                                 # terms that carry a planted scalar and stay alive
    info = {"identity": [], "boundary": [], "cover": []}
    cover = cover_scalars(c)
    bsums = sorted({s for lo, cnt in passes(n, m, c) for s in (lo, lo + cnt - 1)})
    if m >= len(cover):
        info["cover"] = cover
        for s in bsums:
            k[s * m:s * m + len(cover)] = dc.scalars(cover, halved=True)
            keep[s * m:s * m + len(cover)] = True
            info["boundary"].append(s)
    interior = [s for s in range(n) if s not in bsums]
    kv = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % R
    if interior:
        b = interior[0] * m
        for j, v in enumerate([0, 1, R - 1, R, (1 << 256) - 1][:m]):
            k[b + j] = _scalar_bytes(v)
        if m > 5:
            dead[b + 5] = True
        if m > 7:
            pts[b + 7] = pts[b + 6]
            keep[b + 6:b + 8] = True
        if m > 9:
            pts[b + 9] = pts[b + 8]
            k[b + 8], k[b + 9] = _scalar_bytes(kv), _scalar_bytes(R - kv)
            keep[b + 8:b + 10] = True
    if len(interior) > 1:
        s = interior[1]
        dead[s * m:(s + 1) * m] = True
        info["identity"].append(s)
    if len(interior) > 2 and m >= 2:
        s = interior[2]
        k[s * m:(s + 1) * m] = 0
        pts[s * m + m - 1] = pts[s * m]
        k[s * m], k[s * m + m - 1] = _scalar_bytes(kv), _scalar_bytes(R - kv)
        keep[s * m:(s + 1) * m] = True
        info["identity"].append(s)
    ninth = np.zeros(terms, bool)
    ninth[8::9] = True
    dead |= ninth & ~keep
    info["dead"] = dead
    if encoded:
        enc = oracle.compress(pts)
        enc[dead, 31] |= 0x40
        return enc, k, info
    if projective:                                               # the last sum as the map left it: Z != 1
        lo = (n - 1) * m
        keepers = np.array([(pts[j] == pts[j - 1]).all() for j in range(lo, terms)])      # (none: the last sum is a boundary sum)
        assert not keepers.any()
        pts[lo:] = mapped[lo:]
        assert (pts[lo:, 8:12] != pts[0, 8:12]).any(axis=1).all() and (pts[:lo, 8:12] == pts[0, 8:12]).all()
    rec = pts.reshape(terms, 4, 4)
    rec[dead, 2] = 0                                             # Z = 0: no group element, counts as the identity
    return np.ascontiguousarray(rec.reshape(terms, 16)), k, info


def live_scalars_of_sum(k, info, m, s):
    """The values k / 2 mod r that the live terms of sum s walk (what the digits are taken from)."""
    inv2 = (R + 1) // 2
    out = []
    for j in range(s * m, (s + 1) * m):
        if not info["dead"][j]:
            out.append(int.from_bytes(k[j].tobytes(), "little") % R * inv2 % R)
    return out


def assert_boundary_sums_cover(k, info, m, c):
    """Every claimed pair of the layout is reached by the live terms of every boundary sum; no pair is left out."""
    layout = dc.msm(c)
    assert info["boundary"], "m holds the cover scalars"
    for s in info["boundary"]:
        dc.assert_covers(layout, live_scalars_of_sum(k, info, m, s))
