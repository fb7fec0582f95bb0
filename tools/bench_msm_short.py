#!/usr/bin/env python3
"""The one long sum over short scalars (d377_msm_short_dev, include/decaf377_amd_short_msm.h) against d377_msm_dev on the same
values zero-extended to 32 bytes, in one process on one device, Element records, for 8- and 16-byte scalars.  The method is
tools/bench_bucket_sums.py's: every leg on torch tensors that live on the device, timed from the call to the end of a device
synchronise; the legs ALTERNATE round by round; the median of the timed rounds is reported with each leg's min-to-max spread,
and the Encodings of the legs must be equal.  A leg is "ahead" only where the medians differ by more than the two spreads
together.
    python tools/bench_msm_short.py [--reps 5] [--warmup 2]   ->  profiles/msm_short_bench.json: n = 2^12, 2^16, 2^20, 2^22
    python tools/bench_msm_short.py --sweep                   ->  profiles/msm_short_window_sweep.txt: D377_TUNE_MSM_WINDOW swept at
                                                                  2^16, 2^20, 2^22 for both lengths (the short form alone)
    python tools/bench_msm_short.py --small                   ->  printed: n = 256, 1024, 3072, the short form (buckets) against
                                                                  d377_msm_dev on its own routes (waves) and on the buckets
    python tools/bench_msm_short.py --trace                   ->  a few calls of each form at 2^20 and nothing else: the program to
                                                                  put behind a kernel trace for the cost of the final stage
    python tools/bench_msm_short.py --scale 8                 (every n divided by 2^8, printed and not written)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import decaf377_amd as d  # noqa: E402
from bench_bucket_sums import summary, timed  # noqa: E402

SIZES = (1 << 12, 1 << 16, 1 << 20, 1 << 22)
SWEEP_SIZES = (1 << 16, 1 << 20, 1 << 22)
SWEEP_WIDTHS = range(10, 17)
SMALL = (256, 1024, 3072)


def verdict(a, b, name_a, name_b):
    """which of two summaries is ahead by more than both spreads together, or None"""
    gap = b["median_ms"] - a["median_ms"]
    if abs(gap) <= a["spread_ms"] + b["spread_ms"]:
        return None
    return name_a if gap > 0 else name_b


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=0, help="divide every n by 2^SCALE (a rehearsal: printed and not written)")
    ap.add_argument("--sweep", action="store_true", help="sweep the window width of the short form")
    ap.add_argument("--small", action="store_true", help="the sizes of d377_msm's wave routes")
    ap.add_argument("--trace", action="store_true", help="a few calls at 2^20 for a kernel trace")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = d.Context([0], comb_lazy=True)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(20)
    rnd = lambda rows, cols: torch.randint(0, 256, (rows, cols), dtype=torch.uint8, device=dev, generator=gen)   # noqa: E731
    top = (SMALL[-1] if a.small else (1 << 20) if a.trace else max(SIZES)) >> (0 if a.small else a.scale)
    pts = ctx.decompress(ctx.encode_to_curve(rnd(top, 32)))[0].contiguous()
    rec16 = rnd(top, 16)
    short = {16: rec16, 8: rec16[:, :8].contiguous()}
    full = {}
    for nb, r in short.items():
        full[nb] = torch.zeros((top, 32), dtype=torch.uint8, device=dev)
        full[nb][:, :nb] = r
    name = torch.cuda.get_device_name(0)

    if a.trace:
        for _ in range(4):
            for nb in (8, 16):
                ctx.msm_short(pts, short[nb])
                ctx.msm(pts, full[nb])
        torch.cuda.synchronize()
        ctx.close()
        return

    if a.small:
        for nb in (8, 16):
            for n in SMALL:
                p, s, f = pts[:n], short[nb][:n], full[nb][:n]

                def on_buckets():
                    with ctx.tuning(msm_small_max=0):
                        return ctx.msm(p, f)[0]
                legs = [("short", lambda: ctx.msm_short(p, s)[0]), ("msm", lambda: ctx.msm(p, f)[0]), ("msm_buckets", on_buckets)]
                times, out = timed(legs, a.warmup, a.reps)
                assert all((o.cpu() == out["short"].cpu()).all() for o in out.values()), (nb, n)
                case = {"scalar_bytes": nb, "n": n, **{k: summary(v) for k, v in times.items()}}
                case["ahead"] = verdict(case["short"], case["msm"], "short", "msm")
                print(json.dumps(case), flush=True)
        ctx.close()
        return

    if a.sweep:
        lines = ["# d377_msm_short_dev, D377_TUNE_MSM_WINDOW swept, Element records, %s" % name,
                 "# median of %d after %d warm-ups, ms to the end of a device synchronise (min .. max); the widths of one (length, n)" % (a.reps, a.warmup),
                 "# alternate in one process; asked = the override, used x windows = what the plan made of it; rule = pick_window's width by n"]
        for nb in (8, 16):
            for n in SWEEP_SIZES:
                n >>= a.scale
                p, s = pts[:n], short[nb][:n]
                rule = ctx.msm_short_plan(n, nb)

                def leg(c):
                    with ctx.tuning(msm_window=c):
                        return ctx.msm_short(p, s)[0]
                legs = [("c%d" % c, (lambda c=c: leg(c))) for c in SWEEP_WIDTHS]
                times, out = timed(legs, a.warmup, a.reps)
                ref = out[legs[0][0]].cpu()
                assert all((o.cpu() == ref).all() for o in out.values()), (nb, n)
                for c in SWEEP_WIDTHS:
                    with ctx.tuning(msm_window=c):
                        plan = ctx.msm_short_plan(n, nb)
                    sm = summary(times["c%d" % c])
                    lines.append("bytes %2d  n %8d  asked %2d  used %2d x %2d  %9.3f  (%9.3f .. %9.3f)%s" % (
                        nb, n, c, plan["window_bits"], plan["windows"], sm["median_ms"], sm["min_ms"], sm["max_ms"],
                        "  <- rule" if (plan["window_bits"], plan["windows"]) == (rule["window_bits"], rule["windows"]) else ""))
                print("\n".join(lines[-len(legs):]), flush=True)
        if not a.scale:
            with open(a.out or os.path.join(root, "profiles", "msm_short_window_sweep.txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
        ctx.close()
        return

    rec = {"device": name, "reps": a.reps, "warmup": a.warmup,
           "method": "the legs alternate round by round; median of the timed rounds, spread = max - min; Element records and scalars on "
                     "the device, timed to the end of a device synchronise; a leg is ahead only where the medians differ by more than "
                     "the two spreads together",
           "legs": {"short": "d377_msm_short_dev", "msm": "d377_msm_dev on the same values zero-extended to 32 bytes"},
           "cases": []}
    for nb in (8, 16):
        for n in SIZES:
            n >>= a.scale
            p, s, f = pts[:n], short[nb][:n], full[nb][:n]
            times, out = timed([("short", lambda: ctx.msm_short(p, s)[0]), ("msm", lambda: ctx.msm(p, f)[0])], a.warmup, a.reps)
            equal = bool((out["short"].cpu() == out["msm"].cpu()).all())
            assert equal, (nb, n)
            case = {"scalar_bytes": nb, "n": n, "plan": ctx.msm_short_plan(n, nb), "encodings_equal": equal,
                    "short": summary(times["short"]), "msm": summary(times["msm"])}
            case["ahead"] = verdict(case["short"], case["msm"], "short", "msm")
            case["ratio_msm_over_short"] = round(case["msm"]["median_ms"] / case["short"]["median_ms"], 3)
            rec["cases"].append(case)
            print(json.dumps(case), flush=True)
    if not a.scale:
        with open(a.out or os.path.join(root, "profiles", "msm_short_bench.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
