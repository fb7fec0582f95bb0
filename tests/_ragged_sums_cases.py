"""The cases that tests/test_ragged_sums_host.py and tests/test_ragged_sums_gpu.py share: the plan of d377_batch_ragged_msm as
include/decaf377_amd_ragged_sums.h and decaf377_amd/csrc/msm_ragged_plan.hpp state it in words (restated here, independent of
the header's code), the oracle's fold per sum, and the builder of the planted cases."""
import numpy as np

import _digit_cases as dc
from _bucket_sums_cases import cover_scalars, oracle_fold, window_rule
from _sums_support import scalar_bytes as _scalar_bytes

R = dc.R
MAX_TERMS = 1 << 20
MAX_KEYS = 1 << 17
MAX_POINTS = 1 << 24

# The GPU cases: name -> (lengths, window_bits).
ALT17 = tuple(40 + (i & 1) for i in range(17))
CASES = {
    "passes_middle_empty": ((40, 0, 3, 1, 0, 0, 0, 0, 33), 16),      # c = 16: four sums per pass; the middle pass has no point
    "passes_empty_ends": ((0, 1, 64, 0, 0, 7, 40, 2, 0), 16),        # the call starts and ends with an empty sum
    "tiles_and_waves": ((1,) * 200 + (300,) + (1,) * 70 + (513,), 4),  # > 64 sums in one 256-term tile; a sum across a tile boundary
    "int32_keys": (ALT17, 12),                                       # 17 * 2^11 > 2^15
    "int16_keys": (ALT17[:16], 12),                                  # 16 * 2^11 = 2^15: int16 keys that reach 2^15
}
WIDTH_CASE = ((1, 4096, 17, 600, 0, 2048), 0)                        # the library's width


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.uint64))]).astype(np.uint64)


def lengths_of(off):
    return [int(off[i + 1]) - int(off[i]) for i in range(len(off) - 1)]


def width(off, window_bits=0):
    """A forced width as given; else the uniform call's rule on the mean length max(1, ceil(terms / n))."""
    n = len(off) - 1
    if window_bits:
        return window_bits
    return window_rule(max(1, -(-int(off[n]) // max(n, 1))))


def passes(off, c):
    """[(first sum, sums, points)]: greedy runs of consecutive sums; a pass takes the next sum while (K + 1) 2^(c-1) <= 2^17 and
    points + length <= 2^24."""
    n = len(off) - 1
    out, first = [], 0
    while first < n:
        K = pts = 0
        while first + K < n and ((K + 1) << (c - 1)) <= MAX_KEYS and pts + int(off[first + K + 1]) - int(off[first + K]) <= MAX_POINTS:
            pts += int(off[first + K + 1]) - int(off[first + K])
            K += 1
        assert K >= 1
        out.append((first, K, pts))
        first += K
    return out


def device_cuts(off, devices):
    """The devices + 1 cuts of the host forms' slices: cut k is the sum boundary whose offset is nearest to floor(terms k /
    devices), the lowest such boundary."""
    n = len(off) - 1
    o = [int(v) for v in off]
    cuts = [0]
    for k in range(1, devices):
        t = o[n] * k // devices
        cuts.append(min(range(n + 1), key=lambda j: (abs(o[j] - t), j)))
    return cuts + [n]


def sum_of_term(off, K, g):
    """By a linear scan: the largest k < K with off[k] <= g."""
    return max(k for k in range(K) if int(off[k]) <= g)


def ragged_fold(oracle, points, k, off):
    """oracle_fold per sum, the sums of one length folded together -> (encodings [n, 32], records [n, 16], status or None).  An
    empty sum: the all-zero Encoding and the identity."""
    n = len(off) - 1
    lens = np.array(lengths_of(off))
    enc = np.zeros((n, 32), np.uint8)
    el = np.tile(oracle.identity_xyzt(), (n, 1)).astype(np.uint64)
    status = np.zeros(int(off[n]), np.uint8) if points.shape[1] == 32 else None
    for L in sorted(set(lens.tolist()) - {0}):
        sums = np.nonzero(lens == L)[0]
        idx = np.concatenate([np.arange(int(off[s]), int(off[s + 1])) for s in sums])
        e, x, st = oracle_fold(oracle, np.ascontiguousarray(points[idx]), np.ascontiguousarray(k[idx]), L)
        enc[sums], el[sums] = e, x
        if status is not None:
            status[idx] = st
    return enc, el, status


def make_case(oracle, rng, lengths, c, encoded=False):
    """Sums of the given lengths for window width c -> (points, scalars, offsets, info).  With t = len(cover_scalars(c)):
      the first and the last sum of every pass that holds t + 2 terms   the cover scalars on its terms 1 .. t, so that the lowest
                         and the highest bucket of every window of those sums are reached (info["cover_sums"])
      the longest sum    its first and its last term dead; where it holds them, after its terms 0 .. t: scalars 0, 1, r - 1, r,
                         2^256 - 1, one point on two terms, k P and (r - k) P
      every 9th term of the call   dead, unless it carries a planted scalar
    Element records have Z = 1; a dead Element record has Z = 0, a dead Encoding bit 0x40 of byte 31."""
    off = offsets_of(lengths)
    n, terms = len(lengths), int(off[-1])
    pts = np.ascontiguousarray(oracle.decompress(oracle.compress(oracle.elligator_map_xyzt(
        rng.integers(0, 256, (terms, 32), dtype=np.uint8))))[0], dtype=np.uint64)
    k = rng.integers(0, 256, (terms, 32), dtype=np.uint8)
    dead, keep = np.zeros(terms, bool), np.zeros(terms, bool)
    cover = cover_scalars(c)
    t = len(cover)
    info = {"cover_sums": [], "cover": cover, "empty": [s for s in range(n) if lengths[s] == 0]}
    for first, K, _ in passes(off, c):
        fit = [s for s in range(first, first + K) if lengths[s] >= t + 2]
        for s in sorted(set(fit[:1] + fit[-1:])):
            b = int(off[s]) + 1
            k[b:b + t] = dc.scalars(cover, halved=True)
            keep[b:b + t] = True
            info["cover_sums"].append(s)
    big = int(np.argmax(lengths))
    b, L = int(off[big]), lengths[big]
    if L >= 1:
        dead[b] = dead[b + L - 1] = True
        keep[b] = keep[b + L - 1] = True                         # (their fate is settled)
    if L >= t + 11:
        p = b + t + 1
        for j, v in enumerate([0, 1, R - 1, R, (1 << 256) - 1]):
            k[p + j] = _scalar_bytes(v)
        pts[p + 6] = pts[p + 5]
        kv = int.from_bytes(rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), "little") % R
        pts[p + 8] = pts[p + 7]
        k[p + 7], k[p + 8] = _scalar_bytes(kv), _scalar_bytes(R - kv)
        keep[p:p + 9] = True
        info["specials"] = p
    ninth = np.zeros(terms, bool)
    ninth[8::9] = True
    dead |= ninth & ~keep
    info["dead"] = dead
    if encoded:
        enc = oracle.compress(pts)
        enc[dead, 31] |= 0x40
        return enc, k, off, info
    rec = pts.reshape(terms, 4, 4)
    rec[dead, 2] = 0
    return np.ascontiguousarray(rec.reshape(terms, 16)), k, off, info


def assert_cover_sums_cover(k, off, info, c):
    """Every claimed (window, digit) pair of the layout is reached by the live terms of every cover sum."""
    layout = dc.msm(c)
    inv2 = (R + 1) // 2
    assert info["cover_sums"], "some sum holds the cover scalars"
    for s in info["cover_sums"]:
        live = [int.from_bytes(k[j].tobytes(), "little") % R * inv2 % R for j in range(int(off[s]), int(off[s + 1])) if not info["dead"][j]]
        dc.assert_covers(layout, live)
