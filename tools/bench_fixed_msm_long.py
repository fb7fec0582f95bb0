#!/usr/bin/env python3
"""d377_batch_fixed_long_msm against what a caller had before it: n sums over the SAME m registered bases
  (a) as ONE call of d377_batch_fixed_long_msm on a registration of d377_fixed_bases_create_long,
  (b) as d377_batch_msm_long on the same sums with the m bases tiled n times,
  (c) as the composition available before: d377_batch_fixed_msm on handles of 64 bases with Element records out, rounds of
      d377_batch_add, one d377_batch_compress  (m > 64),
  (d) as d377_msm, for a single sum (n = 1),
  (e) as d377_batch_fixed_msm itself on a short registration (m <= 64): there the new call's only difference is the cut.
All on host (numpy) arrays -- the fixed-base calls are host-pointer only -- in one process on one device, wall-clock per call
(every host-pointer call returns synchronised), warm-up calls before the timed ones, the median of the timed ones reported.
Every case records the cut (FixedBases.long_plan), the comb bytes and the mixed additions per second of leg (a), terms x W /
median, next to the 1.68e10 of the indexed kernel over 4.3 GB of combs (profiles/fixed_bases_indexed_bench.json); "a_loses"
lists every leg that beat the new call.
    python tools/bench_fixed_msm_long.py [--reps 5] [--warmup 2]   ->  profiles/fixed_msm_long_bench.json, one JSON line per shape
    python tools/bench_fixed_msm_long.py --only "4096,256,12;256,4096,8" --legs a      (chosen shapes, the new call alone, printed and not written:
        for `rocprofv3 --kernel-trace --stats -- python ...`, and for A/B builds of the library loaded through D377_LIB --
        -DD377_FML_SEG_MIN=2 / 4, -DD377_FML_SUM_MAJOR)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import decaf377_amd as d

SHAPES = [(1 << 12, 256, 12), (1 << 8, 4096, 8), (1 << 8, 4096, 12), (1 << 16, 65, 12), (1, 4096, 8), (256, 64, 16)]
WINDOWS = {8: 32, 12: 21, 16: 16, 18: 14}


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "reps": reps}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "fixed_msm_long_bench.json"))
    ap.add_argument("--only", default=None, help="n,m,bits[;n,m,bits ...]: those shapes, printed and not written")
    ap.add_argument("--legs", default="abcde", help="which legs to time (a is always run)")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in one.split(",")) for one in a.only.split(";")] if a.only else SHAPES
    ctx = d.Context([0], comb_lazy=True)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(12)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "path": "host (numpy)",
           "library": os.environ.get("D377_LIB") or "default build",
           "legs": {"a": "d377_batch_fixed_long_msm", "b": "d377_batch_msm_long, bases tiled",
                    "c": "d377_batch_fixed_msm on 64-base handles + rounds of d377_batch_add + d377_batch_compress",
                    "d": "d377_msm (n = 1)", "e": "d377_batch_fixed_msm on a short handle (m <= 64)"},
           "indexed_kernel_additions_per_sec": 1.68e10, "cases": [], "a_loses": []}
    for n, m, bits in shapes:
        terms = n * m
        r0 = torch.randint(0, 256, (m, 32), dtype=torch.uint8, device=dev, generator=gen)
        B = ctx.decompress(ctx.encode_to_curve(r0))[0].cpu().numpy().view(np.uint64)
        k = torch.randint(0, 256, (terms, 32), dtype=torch.uint8, device=dev, generator=gen).cpu().numpy()
        fb = ctx.fixed_bases_long(B, comb_bits=bits)
        g, b = fb.long_plan(n)
        got = fb.msm_long(k)
        ta = timed(lambda: fb.msm_long(k), a.warmup, a.reps)
        case = {"n": n, "m": m, "comb_bits": bits, "terms": terms, "segments": g, "bases_per_segment": b,
                "comb_bytes": fb.table_bytes, "a_fixed_msm_long": ta,
                "a_terms_per_sec": round(terms / (ta["median_ms"] * 1e-3)),
                "a_additions_per_sec": round(terms * WINDOWS[bits] / (ta["median_ms"] * 1e-3))}
        others = {}
        if "b" in a.legs and 9 <= m:
            P = np.ascontiguousarray(np.tile(B, (n, 1)))
            assert (ctx.msm_long(P, k, m) == got).all(), (n, m, bits)
            others["b_msm_long_tiled"] = timed(lambda: ctx.msm_long(P, k, m), a.warmup, a.reps)
            del P
        if "c" in a.legs and m > 64:
            parts = [(lo, min(lo + 64, m)) for lo in range(0, m, 64)]
            handles = [ctx.fixed_bases(B[lo:hi], comb_bits=bits) for lo, hi in parts]
            k3 = k.reshape(n, m, 32)
            ks = [np.ascontiguousarray(k3[:, lo:hi]).reshape(-1, 32) for lo, hi in parts]   # (a caller would hold them so)

            def composed():
                xs = [h.msm(kk, elements=True)[1] for h, kk in zip(handles, ks)]
                while len(xs) > 1:
                    half = len(xs) // 2
                    s = ctx.add(np.concatenate(xs[:half]), np.concatenate(xs[half:2 * half]))
                    xs = [s[i * n:(i + 1) * n] for i in range(half)] + xs[2 * half:]
                return ctx.compress(xs[0])

            assert (composed() == got).all(), (n, m, bits)
            others["c_composition"] = timed(composed, a.warmup, a.reps)
            for h in handles:
                h.close()
        if "d" in a.legs and n == 1:
            assert (ctx.msm(B, k)[0] == got[0]).all()
            others["d_msm"] = timed(lambda: ctx.msm(B, k), a.warmup, a.reps)
        if "e" in a.legs and m <= 64:
            with ctx.fixed_bases(B, comb_bits=bits) as short:
                assert (short.msm(k) == got).all()
                others["e_fixed_msm"] = timed(lambda: short.msm(k), a.warmup, a.reps)
        for name, t in others.items():
            case[name] = t
            case[name[0] + "_over_a"] = round(t["median_ms"] / ta["median_ms"], 2)
            if t["median_ms"] < ta["median_ms"]:
                rec["a_loses"].append({"n": n, "m": m, "comb_bits": bits, "to": name[0]})
        fb.close()
        rec["cases"].append(case)
        print(json.dumps(case), flush=True)
    for lost in rec["a_loses"]:
        print("d377_batch_fixed_long_msm is SLOWER than leg (%s) at (n, m, bits) = (%d, %d, %d)" % (lost["to"], lost["n"], lost["m"], lost["comb_bits"]), flush=True)
    if not a.only:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
