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

`--indexed` runs the other leg instead, d377_batch_fixed_msm_indexed against d377_batch_fixed_msm (profiles/
fixed_bases_indexed_bench.json), same conventions:

  what indexing buys    m = 64 bases x comb_bits in {12, 16} x t in {1, 2, 4, 8} terms x n in {2^12, 2^20}: t distinct random
                        bases per sum, against the dense call on the same sums (zero scalars elsewhere); m / t is the ratio by
                        addition count
  what indexing costs   m = t = 8, index row 0 .. 7, 16 bits, 2^20 sums, against the dense call on the same scalars: the same
                        additions plus the index traffic
  with --indexed, --only takes cases m,bits,t,n

usage: tools/fixed_bases_bench.py [--indexed] [--quick] [--only m,bits,n[;...]] [--reps 5] [--warmup 2] [--out FILE]"""
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


def indexed_leg(a, d, ctx, orc, rng, torch):
    """d377_batch_fixed_msm_indexed against d377_batch_fixed_msm on the same sums."""
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    cases = [(64, bits, t, n) for bits in (12, 16) for n in (1 << 12, 1 << 20) for t in (1, 2, 4, 8)] + [(8, 16, 8, 1 << 20)]
    if a.only:
        cases = [tuple(int(x) for x in c.split(",")) for c in a.only.split(";")]
    pts = np.concatenate([orc.generator_xyzt().reshape(1, 16),
                          orc.elligator_map_xyzt(rng.integers(0, 256, (63, 32), dtype=np.uint8))]).astype(np.uint64)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "path": "host (numpy)", "cases": []}
    fb, key = None, None
    for m, bits, t, n in cases:
        if key != (m, bits):
            if fb is not None:
                fb.close()
            fb, key = ctx.fixed_bases(pts[:m], comb_bits=bits), (m, bits)
        lib, c, h = fb._lib, ctx._h, fb._h
        if t == m:                                                # what indexing costs: every base, in registration order
            idx = np.ascontiguousarray(np.tile(np.arange(m, dtype=np.int32), (n, 1)))
        else:                                                     # what it buys: t distinct bases per sum
            idx = np.ascontiguousarray(np.argsort(rng.random((n, m)), axis=1)[:, :t].astype(np.int32))
        k = rng.integers(0, 256, (n, t, 32), dtype=np.uint8)
        dense = np.zeros((n, m, 32), np.uint8)
        dense[np.arange(n)[:, None], idx] = k
        enc_d, enc_i = np.empty((n, 32), np.uint8), np.empty((n, 32), np.uint8)
        rd = timed(lambda: d._native.check(lib.d377_batch_fixed_msm(c, h, p(dense), ctypes.c_size_t(n), p(enc_d), None)), a.warmup, a.reps)
        ri = timed(lambda: d._native.check(lib.d377_batch_fixed_msm_indexed(c, h, p(idx), p(k), ctypes.c_size_t(t), ctypes.c_size_t(n),
                                                                            p(enc_i), None)), a.warmup, a.reps)
        assert (enc_d == enc_i).all()
        r = {"m": m, "bits": bits, "t": t, "n": n, "dense": rd, "indexed": ri,
             "dense_over_indexed": round(rd["median_ms"] / ri["median_ms"], 2), "by_addition_count": round(m / t, 2),
             "indexed_median_inside_dense_min_max": rd["min_ms"] <= ri["median_ms"] <= rd["max_ms"],
             "host_bytes_in_dense": n * m * 32, "host_bytes_in_indexed": n * t * 36}
        rec["cases"].append(r)
        print(json.dumps(r), flush=True)
        del dense
    if fb is not None:
        fb.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--indexed", action="store_true", help="d377_batch_fixed_msm_indexed against the dense call (cases m,bits,t,n)")
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
    if a.indexed:
        rec = indexed_leg(a, d, ctx, orc, rng, torch)
        ctx.close()
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(rec, indent=1) + "\n")
        print("FIXED_BASES_BENCH_OK")
        return
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
