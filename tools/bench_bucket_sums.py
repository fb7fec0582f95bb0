#!/usr/bin/env python3
"""Many sums by the bucket method (d377_batch_bucket_msm_resident, include/decaf377_amd_bucket_sums.h) against the calls it
stands beside, in one process on one device, 2^20 terms per call at (n, m) = (2^12, 256), (2^8, 4096), (2^4, 2^16), (1, 2^20).
Legs, all on torch tensors that live on the device, each timed from the call to the end of a device synchronise:
  buckets   d377_batch_bucket_msm_resident, the library's window width
  straus    d377_batch_long_msm_resident (m <= 4096 only)
  msm       n calls of d377_msm_dev on one stream
The legs ALTERNATE: after the warm-up rounds every round times each leg once; the median of the rounds is reported with each
leg's min-to-max spread, and the Encodings of the legs must be equal.  "buckets_ahead" is true where its median is ahead of
BOTH other legs by more than the two spreads together; anything else is not established or names the leg that is ahead.
    python tools/bench_bucket_sums.py [--reps 5] [--warmup 2]    ->  profiles/bucket_sums_bench.json, one JSON line per shape
    python tools/bench_bucket_sums.py --sweep                    ->  profiles/bucket_sums_window_sweep.txt: window_bits swept at
                                                                     m = 256, 4096, 2^16, 2^20 (2^20 terms per call), the Straus leg beside it,
                                                                     and the rule's width at m = 512, 1024, 2048
    python tools/bench_bucket_sums.py --scale 8                  (every n divided by 2^8, printed and not written)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: F401,E402
import torch  # noqa: E402
import decaf377_amd as d  # noqa: E402

SHAPES = [(1 << 12, 256), (1 << 8, 4096), (1 << 4, 1 << 16), (1, 1 << 20)]
SWEEP = {256: range(4, 11), 4096: range(6, 14), 1 << 16: range(9, 17), 1 << 20: range(13, 17)}
CROSSOVER = (512, 1024, 2048)                                  # between the swept 256 and 4096: the rule's width against the Straus leg


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
            "spread_ms": round(max(ts) - min(ts), 3), "reps": len(ts)}


def timed(legs, warmup, reps):
    """legs: [(name, fn)] -> ({name: [ms]}, {name: last output}); the legs alternate round by round."""
    times, out = {name: [] for name, _ in legs}, {}
    torch.cuda.synchronize()
    for r in range(warmup + reps):
        for name, fn in legs:
            t0 = time.perf_counter()
            out[name] = fn()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return times, out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=0, help="divide every n by 2^SCALE (a rehearsal: printed and not written)")
    ap.add_argument("--sweep", action="store_true", help="sweep window_bits instead of comparing the legs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = d.Context([0], comb_lazy=True)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(20)
    rnd = lambda rows: torch.randint(0, 256, (rows, 32), dtype=torch.uint8, device=dev, generator=gen)   # noqa: E731
    points = lambda rows: ctx.decompress(ctx.encode_to_curve(rnd(rows)))[0]                                # noqa: E731
    terms = (1 << 20) >> a.scale
    pts, k = points(terms).contiguous(), rnd(terms)

    if a.sweep:
        lines = ["# d377_batch_bucket_msm_resident, window_bits swept, %d terms per call, %s" % (terms, torch.cuda.get_device_name(0)),
                 "# median of %d after %d warm-ups, ms to the end of a device synchronise (min .. max); rule = the width the library picks;" % (a.reps, a.warmup),
                 "# straus = d377_batch_long_msm_resident on the same inputs in the same rounds (m <= 4096)"]
        for m, widths in SWEEP.items():
            n = terms // m
            rule = ctx.msm_buckets_plan(n, m)["window_bits"]
            legs = [("c%d" % c, (lambda c=c: ctx.msm_buckets(pts, k, m, window_bits=c))) for c in widths]
            if m <= 4096:
                legs.append(("straus", lambda: ctx.msm_long(pts, k, m)))
            times, out = timed(legs, a.warmup, a.reps)
            ref = out[legs[0][0]].cpu()
            assert all((o.cpu() == ref).all() for o in out.values()), m
            for name, _ in legs:
                s = summary(times[name])
                plan = ctx.msm_buckets_plan(n, m, int(name[1:])) if name != "straus" else None
                lines.append("n %6d  m %7d  %-6s %9.3f  (%9.3f .. %9.3f)%s%s" % (
                    n, m, name, s["median_ms"], s["min_ms"], s["max_ms"],
                    "  passes %d  workspace %.2f GB" % (plan["passes"], plan["workspace_bytes"] / 2 ** 30) if plan else "",
                    "  <- rule" if name == "c%d" % rule else ""))
            print("\n".join(lines[-len(legs):]), flush=True)
        lines.append("# the crossover against d377_batch_long_msm_resident: the rule's width at the lengths between")
        for m in CROSSOVER:
            n = terms // m
            times, out = timed([("buckets", lambda: ctx.msm_buckets(pts, k, m)), ("straus", lambda: ctx.msm_long(pts, k, m))], a.warmup, a.reps)
            assert (out["buckets"].cpu() == out["straus"].cpu()).all(), m
            sb, ss = summary(times["buckets"]), summary(times["straus"])
            lines.append("n %6d  m %7d  c%-5d %9.3f  (%9.3f .. %9.3f)   straus %9.3f  (%9.3f .. %9.3f)" % (
                n, m, ctx.msm_buckets_plan(n, m)["window_bits"], sb["median_ms"], sb["min_ms"], sb["max_ms"], ss["median_ms"], ss["min_ms"], ss["max_ms"]))
            print(lines[-1], flush=True)
        if not a.scale:
            with open(a.out or os.path.join(root, "profiles", "bucket_sums_window_sweep.txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
        ctx.close()
        return

    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "terms_per_call": terms,
           "method": "the legs alternate round by round; median of the timed rounds, spread = max - min; every leg on device tensors, "
                     "timed to the end of a device synchronise; buckets_ahead only where its median is ahead of both other legs by "
                     "more than the two spreads together",
           "legs": {"buckets": "d377_batch_bucket_msm_resident, window_bits = 0", "straus": "d377_batch_long_msm_resident (m <= 4096)",
                    "msm": "n calls of d377_msm_dev on one stream"},
           "cases": []}
    for n, m in SHAPES:
        n = max(1, n >> a.scale)
        p, s = pts[:n * m], k[:n * m]
        legs = [("buckets", lambda: ctx.msm_buckets(p, s, m))]
        if m <= 4096:
            legs.append(("straus", lambda: ctx.msm_long(p, s, m)))
        legs.append(("msm", lambda: torch.stack([ctx.msm(p[i * m:(i + 1) * m], s[i * m:(i + 1) * m])[0] for i in range(n)])))
        times, out = timed(legs, a.warmup, a.reps)
        ref = out["buckets"].cpu()
        equal = {name: bool((o.cpu() == ref).all()) for name, o in out.items()}
        assert all(equal.values()), (n, m, equal)
        case = {"n": n, "m": m, "plan": ctx.msm_buckets_plan(n, m), "encodings_equal": equal}
        for name, _ in legs:
            case[name] = summary(times[name])
        b = case["buckets"]
        others = [name for name, _ in legs if name != "buckets"]
        case["buckets_ahead"] = all(case[o]["median_ms"] - b["median_ms"] > case[o]["spread_ms"] + b["spread_ms"] for o in others)
        case["ahead_of_buckets"] = [o for o in others if b["median_ms"] - case[o]["median_ms"] > case[o]["spread_ms"] + b["spread_ms"]]
        rec["cases"].append(case)
        print(json.dumps(case), flush=True)
    if not a.scale:
        with open(a.out or os.path.join(root, "profiles", "bucket_sums_bench.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
