#!/usr/bin/env python3
"""Fixed-base combs for caller-chosen points (d377_fixed_bases_create / d377_batch_fixed_msm): time per call against the
routes a caller had before, on the host path (numpy in, numpy out: every call ends in the library's device synchronise).

  m in {1, 2, 3, 8} x comb_bits in {8, 12, 16, 18} x n sums in {2^12, 2^20, 2^22}    d377_batch_fixed_msm
  the same sums through d377_batch_msm_small (the bases repeated per sum)            m <= 8
  m = 1, bases [GENERATOR], against the context's own 18-bit comb                    d377_batch_scalar_mul_base
  table bytes and creation time per width (m = 1 and m = 3)

Each figure: `--warmup` untimed calls, then `--reps` timed calls; median, min and max ms per call.  Host-path times include
the PCIe copies of scalars and encodings (32 bytes per term in, 32 per sum out; d377_batch_msm_small also copies its
128-byte Element records per term).  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of
`--only` cases (profiles/README.md).

usage: tools/fixed_bases_bench.py [--quick] [--only m,bits,n[;...]] [--reps 5] [--warmup 2] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="n in {2^12, 2^20} only")
    ap.add_argument("--only", default="", help="cases m,bits,n separated by ';' (kernel-trace runs)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import decaf377_amd as d
    from _oracle import Oracle
    assert torch.cuda.is_available(), "fixed_bases_bench needs a GPU"
    orc = Oracle(build=False)
    ctx = d.Context([0], comb_bits=18)
    rng = np.random.default_rng(377)
    gen = orc.generator_xyzt().reshape(1, 16)
    pts = np.concatenate([gen, orc.elligator_map_xyzt(rng.integers(0, 256, (7, 32), dtype=np.uint8))]).astype(np.uint64)
    sizes = [1 << 12, 1 << 20] + ([] if a.quick else [1 << 22])
    cases = [(m, bits, n) for m in (1, 2, 3, 8) for bits in (8, 12, 16, 18) for n in sizes]
    if a.only:
        cases = [tuple(int(x) for x in c.split(",")) for c in a.only.split(";")]
    kmax = max(m * n for m, _, n in cases)
    k = rng.integers(0, 256, (kmax, 32), dtype=np.uint8)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "path": "host (numpy)",
           "tables": [], "fixed_msm": [], "msm_small": [], "context_comb_18": []}
    for bits in (8, 12, 16, 18):
        for m in (1, 3):
            if a.only and not any(c[0] == m and c[1] == bits for c in cases):
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fb = ctx.fixed_bases(pts[:m], comb_bits=bits)
            rec["tables"].append({"m": m, "bits": bits, "create_ms": round((time.perf_counter() - t0) * 1e3, 1),
                                  "bytes_per_device": fb.info()[2], "bytes_per_base": fb.info()[2] // m})
            fb.close()
    small_done = set()
    for m, bits, n in cases:
        with ctx.fixed_bases(pts[:m], comb_bits=bits) as fb:
            enc = np.empty((n, 32), np.uint8)
            sc = k[:m * n]
            lib, c, h = fb._lib, ctx._h, fb._h
            call = lambda: d._native.check(lib.d377_batch_fixed_msm(c, h, sc.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(n),
                                                                    enc.ctypes.data_as(ctypes.c_void_p), None))
            r = timed(call, a.warmup, a.reps)
            r.update({"m": m, "bits": bits, "n": n, "sums_per_s": round(n / r["median_ms"] * 1e3)})
            rec["fixed_msm"].append(r)
            print(json.dumps(r), flush=True)
            if (m, n) not in small_done and m * n <= 1 << 23:     # (the repeated records: 128 bytes per term on both sides)
                small_done.add((m, n))
                rep = np.ascontiguousarray(np.tile(pts[:m], (n, 1)))
                out = np.empty((n, 32), np.uint8)
                r2 = timed(lambda: ctx.msm_small(rep, sc, m, outs=[out]), a.warmup, a.reps)
                r2.update({"m": m, "n": n, "sums_per_s": round(n / r2["median_ms"] * 1e3)})
                rec["msm_small"].append(r2)
                print(json.dumps({"msm_small": r2}), flush=True)
                if m == 1:
                    out1 = np.empty((n, 32), np.uint8)
                    r3 = timed(lambda: ctx.scalar_mul_base(sc, outs=[out1]), a.warmup, a.reps)
                    r3.update({"n": n})
                    rec["context_comb_18"].append(r3)
                    print(json.dumps({"context_comb_18": r3}), flush=True)
    ctx.close()
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print("FIXED_BASES_BENCH_OK")


if __name__ == "__main__":
    main()
