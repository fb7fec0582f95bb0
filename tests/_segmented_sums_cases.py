"""The cases that tests/test_segmented_sums_host.py and tests/test_segmented_sums_gpu.py share, and the plan of
d377_batch_segmented_msm as include/decaf377_amd_segmented_sums.h and decaf377_amd/csrc/msm_segmented_plan.hpp state it in
words, restated here with Python integers and linear scans, independent of the header's code."""
import numpy as np

import _digit_cases as dc
from _ragged_sums_cases import make_case, offsets_of
from _sums_support import scalar_bytes

R = dc.R
MAX_TERMS = 1 << 20
CHAIN = 8                                # terms of a chain
FOLD = 16                                # records a fold lane adds
CHAINS_BELOW_MEAN = 1024                 # advised_route: chains while the mean length of the non-empty sums is below this

# The GPU cases: name -> lengths.
CASES = {
    "crossing_eights": (0, 1, 7, 8, 9, 17, 0, 0, 15, 1, 0),    # one chain; 5 + 4; offsets across multiples of 8; empty sums at both ends and in a run
    "fold_lane_full": (128, 129, 0, 136),                     # g = 16 fills one fold lane; g = 17 needs a slot-indexed level
    "two_levels": (2049, 3),                                  # 257 -> 17 -> 2 -> 1
    "past_long_limit": (4097, 0, 1),                          # past d377_batch_msm_long's 4096
    "many_short": tuple(i % 13 for i in range(300)),          # more sums than one workgroup has lanes
    "ones_and_300": (1,) * 200 + (300,) + (1,) * 70,
    "one_empty": (0,),
    "all_empty": (0, 0, 0),
    "single": (5,),
}
EQUAL = {"equal_24": (24,) * 7, "equal_9": (9,) * 33}         # against msm_long byte for byte


def chains(L):
    return -(-L // CHAIN)


def cut(L):
    """[(first term within the sum, live terms)] of the chains of a sum of L terms: g = ceil(L / 8) chains of b = ceil(L / g)."""
    if L == 0:
        return []
    g = chains(L)
    b = -(-L // g)
    return [(q * b, min(b, L - q * b)) for q in range(g)]


def records(L, level):
    c = chains(L)
    for _ in range(level):
        c = -(-c // FOLD)
    return c


def levels(max_len):
    """Slot-indexed fold levels: while some sum has more than 16 records."""
    c, out = chains(max_len), 0
    while c > FOLD:
        c, out = -(-c // FOLD), out + 1
    return out


def starts(off, level):
    """start_l(i) for every sum: start_0(i) = floor((off[i] - off[0]) / 8) + i, start_{l+1}(i) = floor(start_l(i) / 16) + i."""
    out = [(int(off[i]) - int(off[0])) // CHAIN + i for i in range(len(off) - 1)]
    for _ in range(level):
        out = [s // FOLD + i for i, s in enumerate(out)]
    return out


def space(off, level):
    n = len(off) - 1
    S = (int(off[n]) - int(off[0])) // CHAIN + n
    for _ in range(level):
        S = S // FOLD + n
    return S


def owner(st, p):
    """By a linear scan: the largest i with start(i) <= p (0 if there is none)."""
    return max([i for i, s in enumerate(st) if s <= p], default=0)


def plan(off):
    n = len(off) - 1
    lens = [int(off[i + 1]) - int(off[i]) for i in range(n)]
    nonempty = [L for L in lens if L]
    lv = levels(max(lens, default=0))
    sp = [space(off, l) for l in range(lv + 1)]
    return {"terms": sum(lens), "chain_slots": sp[0] if n else 0, "chains": sum(chains(L) for L in lens), "levels": lv,
            "bmax": max((c for L in lens for _, c in cut(L)), default=0), "space": sp, "records": (sum(sp) + n) if n else 0,
            "route": 1 if nonempty and sum(nonempty) >= CHAINS_BELOW_MEAN * len(nonempty) else 0}


def assert_layout(off):
    """What the header claims of the slot spaces: at every level the starts increase strictly, sum i's records end before sum
    i + 1's begin and inside the space, and at most n slots of a level are dead."""
    n = len(off) - 1
    lens = [int(off[i + 1]) - int(off[i]) for i in range(n)]
    for level in range(levels(max(lens, default=0)) + 1):
        st, S = starts(off, level), space(off, level)
        rec = [records(L, level) for L in lens]
        assert all(a < b for a, b in zip(st, st[1:])), level
        assert all(st[i] + rec[i] <= (st[i + 1] if i + 1 < n else S) for i in range(n)), level
        assert 0 <= S - sum(rec) <= n * (level + 1), (level, S, sum(rec))
        if level == 0:
            assert S - sum(rec) <= n


PLANTED = (0, 1, R - 1, R, (1 << 256) - 1)


def build(oracle, rng, lengths, encoded=False):
    """make_case's points and dead terms (tests/_ragged_sums_cases.py, width 4) with the scalars 0, 1, r - 1, r and 2^256 - 1
    planted on the first live terms of the call -> (points, scalars, offsets, dead)."""
    off = offsets_of(lengths)
    terms = int(off[-1])
    if terms == 0:
        return np.zeros((0, 32), np.uint8) if encoded else np.zeros((0, 16), np.uint64), np.zeros((0, 32), np.uint8), off, np.zeros(0, bool)
    pts, k, off, info = make_case(oracle, rng, lengths, 4, encoded=encoded)
    live = np.nonzero(~info["dead"])[0]
    for j, v in zip(live[1::2], PLANTED):                        # (every other live term: several sums and chains get one)
        k[j] = scalar_bytes(v)
    return pts, k, off, info["dead"]
