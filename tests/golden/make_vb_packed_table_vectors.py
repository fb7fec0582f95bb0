#!/usr/bin/env python3
"""Regenerates tests/golden/vb_packed_table_vectors.json from the big-integer model (oracle/d377_model.py): the window
loop's digits given directly (every digit -8 .. 7, digit 0 everywhere, the top digit 1) and whole scalars, on the identity,
the generator and [r - 1] of it.  Inputs and expected outputs only (hex).

Run from the repository root:  python tests/golden/make_vb_packed_table_vectors.py"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import d377_model as m  # noqa: E402


def digit_words(ds):
    """64 signed window digits (ds[63] in {0, 1}) as the 32 bytes the kernels keep them in: one nibble each, d & 15."""
    v = 0
    for i, d in enumerate(ds):
        assert -8 <= d <= 7
        v |= (d & 15) << (4 * i)
    return v.to_bytes(32, "little")


def main():
    rng = random.Random(377)
    pts = {"identity": m.IDENTITY, "generator": m.GENERATOR, "rm1_generator": m.scalar_mul(m.GENERATOR, m.R_ORDER - 1)}
    out = {"generator": "tests/golden/make_vb_packed_table_vectors.py", "points": {k: m.compress(p).hex() for k, p in pts.items()}}
    cyc = [(i % 16) - 8 for i in range(63)]
    digit_sets = [cyc + [0], cyc[::-1] + [1], [0] * 64, [0] * 63 + [1], [-8] * 63 + [1], [7] * 63 + [0], [-8] * 63 + [0],
                  [1] + [0] * 63, [-1] + [0] * 62 + [1]]
    digit_sets += [[rng.randrange(-8, 8) for _ in range(63)] + [rng.randrange(2)] for _ in range(3)]
    dc = []
    for name, p in pts.items():
        for ds in digit_sets:
            k = sum(d * 16 ** i for i, d in enumerate(ds)) % m.R_ORDER
            dc.append({"point": name, "digits": digit_words(ds).hex(), "enc": m.compress(m.scalar_mul(p, k)).hex()})
    out["digit_cases"] = dc
    r = m.R_ORDER
    h8 = 16 ** 62 - 8 * (16 ** 62 - 1) // 15
    scalars = [0, 1, r - 1, r, (1 << 256) - 1, 2 * r, (2 * h8) % r, h8, (2 * (7 * (16 ** 62 - 1) // 15)) % r, 2, r - 2,
               r + 1, (r + 1) // 2, 16 ** 62, 8, 8 * 16, 8 * 16 ** 31, 8 * 16 ** 61]
    scalars += [rng.getrandbits(256) for _ in range(6)]
    sc = []
    for name, p in pts.items():
        for k in scalars:
            kb = k.to_bytes(32, "little")
            sc.append({"point": m.compress(p).hex(), "scalar": kb.hex(), "status": 0,
                       "enc": m.compress(m.scalar_mul(p, m.fr_from_le_bytes_mod_order(kb))).hex()})
    for bad in (b"\xff" * 32, (1).to_bytes(32, "little")):
        assert m.decompress(bad) is None
        sc.append({"point": bad.hex(), "scalar": (5).to_bytes(32, "little").hex(), "status": 1, "enc": bytes(32).hex()})
    out["scalar_cases"] = sc
    with open(os.path.join(ROOT, "tests", "golden", "vb_packed_table_vectors.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
