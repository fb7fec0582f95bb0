#!/usr/bin/env python3
"""Many sums of any length each (d377_batch_ragged_msm_resident, include/decaf377_amd_ragged_sums.h) against the calls it stands
beside, in one process on one device.  The method is tools/bench_bucket_sums.py's: every leg on torch tensors that live on the
device, timed from the call to the end of a device synchronise; the legs ALTERNATE round by round; the median of the rounds is
reported with each leg's min-to-max spread, and the Encodings of the legs must be equal.
  the cost of the lookup   equal lengths at (n, m) = (2^8, 4096) and (2^4, 2^16): "ragged" against "buckets"
                           (d377_batch_bucket_msm_resident, which shares every kernel but the keys kernel) on the same buffers.
                           "within_spreads" where the medians differ by less than the two spreads together.
  skewed lengths           2^20 terms in lengths doubling from 2^10 to 2^16 and repeating: "ragged" against "padded" (the
                           uniform bucket call on every sum padded to 2^16 terms with dead records) and "msm" (one d377_msm_dev
                           per sum on one stream).  "ragged_ahead" only where its median is ahead of BOTH by more than the two
                           spreads together; anything else is not established or names the leg that is ahead.
    python tools/bench_ragged_sums.py [--reps 5] [--warmup 2]    ->  profiles/ragged_sums_bench.json
    python tools/bench_ragged_sums.py --sweep                    ->  profiles/ragged_sums_window_sweep.txt: window_bits swept on the
                                                                     skewed shape, the mean-length rule's width marked
    python tools/bench_ragged_sums.py --scale 8                  (every length divided by 2^8, printed and not written)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import decaf377_amd as d  # noqa: E402
from bench_bucket_sums import summary, timed  # noqa: E402

EQUAL = [(1 << 8, 4096), (1 << 4, 1 << 16)]
SWEEP = range(8, 15)


def skewed(terms, lo, hi):
    """Lengths doubling from lo to hi and repeating until `terms` are used up (the last one cut to fit)."""
    out, m = [], lo
    while terms:
        out.append(min(m, terms))
        terms -= out[-1]
        m = lo if m == hi else 2 * m
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=0, help="divide every length by 2^SCALE (a rehearsal: printed and not written)")
    ap.add_argument("--sweep", action="store_true", help="sweep window_bits on the skewed shape instead of comparing the legs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = d.Context([0], comb_lazy=True)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(20)
    rnd = lambda rows: torch.randint(0, 256, (rows, 32), dtype=torch.uint8, device=dev, generator=gen)   # noqa: E731
    points = lambda rows: ctx.decompress(ctx.encode_to_curve(rnd(rows)))[0]                                # noqa: E731
    terms = (1 << 20) >> a.scale
    pts, k = points(terms).contiguous(), rnd(terms)
    on_dev = lambda off: torch.from_numpy(off.view(np.int64)).to(dev)                                     # noqa: E731

    lengths = skewed(terms, (1 << 10) >> a.scale, (1 << 16) >> a.scale)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    off_dev = on_dev(off)
    n, longest = len(lengths), max(lengths)

    if a.sweep:
        rule = ctx.msm_ragged_plan(off)["window_bits"]
        lines = ["# d377_batch_ragged_msm_resident, window_bits swept, %d terms in %d sums of %d .. %d terms (doubling, repeating), %s"
                 % (terms, n, min(lengths), longest, torch.cuda.get_device_name(0)),
                 "# median of %d after %d warm-ups, ms to the end of a device synchronise (min .. max); rule = the width of the mean length %d; GB = 10^9 bytes"
                 % (a.reps, a.warmup, -(-terms // n))]
        legs = [("c%d" % c, (lambda c=c: ctx.msm_ragged(pts, k, off, window_bits=c, offsets_dev=off_dev))) for c in SWEEP]
        times, out = timed(legs, a.warmup, a.reps)
        ref = out[legs[0][0]].cpu()
        assert all((o.cpu() == ref).all() for o in out.values())
        for name, _ in legs:
            s, plan = summary(times[name]), ctx.msm_ragged_plan(off, int(name[1:]))
            lines.append("%-4s %9.3f  (%9.3f .. %9.3f)  passes %d  workspace %.2f GB%s" % (
                name, s["median_ms"], s["min_ms"], s["max_ms"], plan["passes"], plan["workspace_bytes"] / 1e9, "  <- rule" if name == "c%d" % rule else ""))
        print("\n".join(lines), flush=True)
        if not a.scale:
            with open(a.out or os.path.join(root, "profiles", "ragged_sums_window_sweep.txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
        ctx.close()
        return

    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "terms_per_call": terms,
           "method": "the legs alternate round by round; median of the timed rounds, spread = max - min; every leg on device tensors, "
                     "timed to the end of a device synchronise; a leg is ahead only where the medians differ by more than the two "
                     "spreads together",
           "legs": {"ragged": "d377_batch_ragged_msm_resident, window_bits = 0, the caller's offsets_dev",
                    "buckets": "d377_batch_bucket_msm_resident, window_bits = 0, on the same buffers (equal lengths)",
                    "padded": "d377_batch_bucket_msm_resident, every sum padded to the longest with dead records (Z = 0, scalar 0)",
                    "msm": "one d377_msm_dev per sum on one stream"},
           "equal_lengths": [], "skewed": None}
    for en, m in EQUAL:
        m = max(1, m >> a.scale)
        eoff = (np.arange(en + 1, dtype=np.uint64) * np.uint64(m)).astype(np.uint64)
        eoff_dev = on_dev(eoff)
        p, s = pts[:en * m], k[:en * m]
        legs = [("ragged", lambda: ctx.msm_ragged(p, s, eoff, offsets_dev=eoff_dev)), ("buckets", lambda: ctx.msm_buckets(p, s, m))]
        times, out = timed(legs, a.warmup, a.reps)
        assert (out["ragged"].cpu() == out["buckets"].cpu()).all(), (en, m)
        case = {"n": en, "m": m, "plan": ctx.msm_ragged_plan(eoff), "uniform_plan": ctx.msm_buckets_plan(en, m), "encodings_equal": True,
                "ragged": summary(times["ragged"]), "buckets": summary(times["buckets"])}
        gap = case["ragged"]["median_ms"] - case["buckets"]["median_ms"]
        case["ragged_minus_buckets_ms"] = round(gap, 3)
        case["within_spreads"] = abs(gap) < case["ragged"]["spread_ms"] + case["buckets"]["spread_ms"]
        rec["equal_lengths"].append(case)
        print(json.dumps(case), flush=True)

    ppts = torch.zeros((n * longest, 16), dtype=pts.dtype, device=dev)        # Z = 0: dead records
    pk = torch.zeros((n * longest, 32), dtype=torch.uint8, device=dev)
    for i, m in enumerate(lengths):
        ppts[i * longest:i * longest + m] = pts[int(off[i]):int(off[i + 1])]
        pk[i * longest:i * longest + m] = k[int(off[i]):int(off[i + 1])]
    legs = [("ragged", lambda: ctx.msm_ragged(pts, k, off, offsets_dev=off_dev)),
            ("padded", lambda: ctx.msm_buckets(ppts, pk, longest)),
            ("msm", lambda: torch.stack([ctx.msm(pts[int(off[i]):int(off[i + 1])], k[int(off[i]):int(off[i + 1])])[0] for i in range(n)]))]
    times, out = timed(legs, a.warmup, a.reps)
    ref = out["ragged"].cpu()
    equal = {name: bool((o.cpu().reshape(ref.shape) == ref).all()) for name, o in out.items()}
    assert all(equal.values()), equal
    case = {"n": n, "terms": terms, "lengths": "%d .. %d doubling, repeating" % (min(lengths), longest), "mean_length": -(-terms // n),
            "plan": ctx.msm_ragged_plan(off), "padded_plan": ctx.msm_buckets_plan(n, longest), "encodings_equal": equal}
    for name, _ in legs:
        case[name] = summary(times[name])
    r = case["ragged"]
    case["ragged_ahead"] = all(case[o]["median_ms"] - r["median_ms"] > case[o]["spread_ms"] + r["spread_ms"] for o in ("padded", "msm"))
    case["ahead_of_ragged"] = [o for o in ("padded", "msm") if r["median_ms"] - case[o]["median_ms"] > case[o]["spread_ms"] + r["spread_ms"]]
    rec["skewed"] = case
    print(json.dumps(case), flush=True)
    if not a.scale:
        with open(a.out or os.path.join(root, "profiles", "ragged_sums_bench.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
