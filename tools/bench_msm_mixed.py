#!/usr/bin/env python3
"""d377_batch_msm_mixed against what a caller had before it: n sums of t terms over registered bases plus v variable points
  (a) as ONE call of d377_batch_msm_mixed,
  (b) as the four-call composition through host memory: d377_batch_msm_small and d377_batch_fixed_msm_indexed with Element
      records out, d377_batch_add, d377_batch_compress.
Both legs on host (numpy) arrays -- the fixed-base calls are host-pointer only -- in one process on one device, wall-clock per
call (every host-pointer call returns synchronised).  The two legs ALTERNATE: after the warm-up rounds every round times (a)
and then (b); the median of the rounds is reported with the min-to-max spread, and the Encodings of the two legs must be equal.
"a_ahead" is true where (b)'s median exceeds (a)'s by more than the two spreads together.
    python tools/bench_msm_mixed.py [--reps 5] [--warmup 2]      ->  profiles/msm_mixed_bench.json, one JSON line per case
    python tools/bench_msm_mixed.py --only "1048576,1,1,1,16" --legs a     (chosen cases n,v,t,bases,bits, printed and not
        written: for `rocprofv3 --kernel-trace --stats -- python ...`, the kernel-only times)"""
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

SHAPES = [(1, 1, 1, 16), (1, 2, 64, 16), (3, 2, 64, 12)]         # (v, t, bases, bits): the signature check, a commitment plus one point
SIZES = [1 << 20, 1 << 12]


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
            "spread_ms": round(max(ts) - min(ts), 3), "reps": len(ts)}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "msm_mixed_bench.json"))
    ap.add_argument("--only", default=None, help="n,v,t,bases,bits[;...]: those cases, printed and not written")
    ap.add_argument("--legs", default="ab", help="which legs to run (a is always run)")
    a = ap.parse_args()
    cases = ([tuple(int(x) for x in one.split(",")) for one in a.only.split(";")] if a.only
             else [(n,) + s for s in SHAPES for n in SIZES])
    ctx = d.Context([0], comb_lazy=True)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(12)
    rnd = lambda rows: torch.randint(0, 256, (rows, 32), dtype=torch.uint8, device=dev, generator=gen)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "path": "host (numpy)",
           "method": "legs alternate round by round; median of the timed rounds, spread = max - min",
           "legs": {"a": "d377_batch_msm_mixed",
                    "b": "d377_batch_msm_small + d377_batch_fixed_msm_indexed (Element records out) + d377_batch_add + d377_batch_compress"},
           "cases": []}
    for n, v, t, m, bits in cases:
        B = ctx.decompress(ctx.encode_to_curve(rnd(m)))[0].cpu().numpy().view(np.uint64)
        P = ctx.decompress(ctx.encode_to_curve(rnd(n * v)))[0].cpu().numpy().view(np.uint64)
        fk, vk = rnd(n * t).cpu().numpy(), rnd(n * v).cpu().numpy()
        idx = torch.randint(0, m, (n, t), dtype=torch.int32, device=dev, generator=gen).cpu().numpy()
        fb = ctx.fixed_bases(B, comb_bits=bits)
        mixed = lambda: fb.msm_mixed(idx, fk, P, vk)

        def composed():
            var_el = ctx.msm_small(P, vk, v, elements=True)[1]
            fix_el = fb.msm_indexed(idx, fk, elements=True)[1]
            return ctx.compress(ctx.add(var_el, fix_el))

        legs = [("a", mixed)] + ([("b", composed)] if "b" in a.legs else [])
        times = {name: [] for name, _ in legs}
        out = {}
        for r in range(a.warmup + a.reps):
            for name, fn in legs:
                t0 = time.perf_counter()
                out[name] = fn()
                if r >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        ta = summary(times["a"])
        case = {"n": n, "v": v, "t": t, "bases": m, "comb_bits": bits, "comb_bytes": fb.table_bytes, "a_msm_mixed": ta,
                "a_sums_per_sec": round(n / (ta["median_ms"] * 1e-3))}
        if "b" in times:
            assert (out["a"] == out["b"]).all(), (n, v, t, m, bits)
            tb = summary(times["b"])
            case["b_composition"] = tb
            case["encodings_equal"] = True
            case["b_over_a"] = round(tb["median_ms"] / ta["median_ms"], 2)
            case["a_ahead"] = bool(tb["median_ms"] - ta["median_ms"] > ta["spread_ms"] + tb["spread_ms"])
            case["b_ahead"] = bool(ta["median_ms"] - tb["median_ms"] > ta["spread_ms"] + tb["spread_ms"])
        fb.close()
        rec["cases"].append(case)
        print(json.dumps(case), flush=True)
    if not a.only:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
