"""The cases that tests/test_msm_long_indexed_host.py and tests/test_msm_long_resident_gpu.py share: a pool of points with a
Z = 0 record, index arrays with the planted absent terms, and the gather materialised for d377_batch_msm_long and the
oracle's fold (tests/_batch_msm_long_cases.py)."""
import numpy as np

from _batch_msm_long_cases import plan
from _sums_support import R, scalar_bytes as _scalar_bytes

POOL = 23
DEAD_RECORD = 5


def make_pool(oracle, rng, count=POOL):
    """`count` Element records; record DEAD_RECORD has Z = 0: no group element, it counts as the identity."""
    pool = np.ascontiguousarray(oracle.elligator_map_xyzt(rng.integers(0, 256, (count, 32), dtype=np.uint8)), dtype=np.uint64)
    pool.reshape(count, 4, 4)[DEAD_RECORD, 2] = 0
    return pool


def make_indexed(rng, n, m, count=POOL):
    """(point_index [n, m] int32, scalars [n m, 32], info).  Planted, where the shape has room:
      the last sum (n > 1)          every term absent: the all-zero Encoding
      sum 0 (m > 1)                 its last term absent
      sum 1 (n > 2, g > 1)          group 0 absent
      n == 1, g > 2                 group 1 absent
    and on the live terms: index 0 on the first, count - 1 on the last, DEAD_RECORD in the middle, a repeat within a sum where
    two neighbours are live, and the scalars 0, 1, r - 1, r, 2^256 - 1 on the first five that are left."""
    g, b = plan(m)
    idx = rng.integers(0, count, (n, m)).astype(np.int32)
    k = rng.integers(0, 256, (n * m, 32), dtype=np.uint8)
    info = {"identity": []}
    if n > 1:
        idx[n - 1, :] = -1
        info["identity"].append(n - 1)
    if m > 1:
        idx[0, m - 1] = -1
    if n > 2 and g > 1:
        idx[1, :b] = -1
    if n == 1 and g > 2:
        idx[0, b:2 * b] = -1
    flat = idx.reshape(-1)
    live = np.nonzero(flat != -1)[0]
    assert len(live) >= 1
    if len(live) >= 5:
        flat[live[len(live) // 2]] = DEAD_RECORD
        a = next((p for p in live[1:-1] if p + 1 in set(live[1:-1]) and p // m == (p + 1) // m and flat[p] != DEAD_RECORD and flat[p + 1] != DEAD_RECORD), None)
        if a is not None:
            flat[a + 1] = flat[a]
            info["repeat"] = int(a)
    flat[live[0]] = 0
    if len(live) > 1:
        flat[live[-1]] = count - 1
    spare = [p for p in live[1:-1] if flat[p] != DEAD_RECORD]
    for p, v in zip(spare, [0, 1, R - 1, R, (1 << 256) - 1]):
        k[p] = _scalar_bytes(v)
    info["absent"] = idx == -1
    return idx, k, info


def materialise(pool, idx):
    """The n m records d377_batch_msm_long takes for the same sums: the gathered pool records, an absent (or refused) term a
    Z = 0 record."""
    flat = np.asarray(idx).reshape(-1).astype(np.int64)
    ok = (flat >= 0) & (flat < len(pool))
    pts = np.zeros((len(flat), 16), np.uint64)
    pts[ok] = pool[flat[ok]]
    return pts
