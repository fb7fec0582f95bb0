#!/usr/bin/env python3
"""Many sums of any length each by Straus chains (d377_batch_segmented_msm_resident, include/decaf377_amd_segmented_sums.h)
against the calls it stands beside, in one process on one device.  The method is tools/bench_bucket_sums.py's: every leg on
torch tensors that live on the device, timed from the call to the end of a device synchronise; the legs ALTERNATE round by
round; the median of the rounds is reported with each leg's min-to-max spread, and the Encodings of the legs must be equal.  A
leg is ahead of another only where the medians differ by more than the two spreads together; the verdict of a pair is "use
this call", "use the other" or "not established".
  (a) the cost of the lookup and of the slot space   equal lengths at (n, m) = (2^16, 16) and (2^12, 256): "segmented" against
                           "long" (d377_batch_long_msm_resident) on the same buffers
  (b) skewed short sums    2^20 terms in lengths doubling from 2 to 2048 and repeating: "segmented" against "ragged"
                           (d377_batch_ragged_msm_resident, the same buffers) and "padded" (d377_batch_long_msm_indexed_resident,
                           every sum padded to 2048 terms with -1)
  (c) the crossover        equal lengths 512, 640, 768, 896, 1024 at 2^20 terms: "long" against "buckets"
                           (d377_batch_bucket_msm_resident).  advised_route's constant is the smallest length at which the
                           buckets are ahead; where none is established it stays at 1024, the point measured before.
    python tools/bench_segmented_sums.py [--reps 5] [--warmup 2]    ->  profiles/segmented_sums_bench.json
    python tools/bench_segmented_sums.py --scale 8                  (2^12 terms per call: a rehearsal, printed and not written)"""
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
from bench_ragged_sums import skewed  # noqa: E402

EQUAL = [(1 << 16, 16), (1 << 12, 256)]
SWEEP = (512, 640, 768, 896, 1024)


def verdict(this, other):
    """Of a pair of summaries: which call to use, by whether the medians differ by more than the two spreads together."""
    gap, room = other["median_ms"] - this["median_ms"], this["spread_ms"] + other["spread_ms"]
    return "use this call" if gap > room else "use the other" if -gap > room else "not established"


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=0, help="divide the terms per call by 2^SCALE (a rehearsal: printed and not written)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = d.Context([0], comb_lazy=True)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(21)
    rnd = lambda rows: torch.randint(0, 256, (rows, 32), dtype=torch.uint8, device=dev, generator=gen)   # noqa: E731
    points = lambda rows: ctx.decompress(ctx.encode_to_curve(rnd(rows)))[0]                                # noqa: E731
    terms = (1 << 20) >> a.scale
    pts, k = points(terms).contiguous(), rnd(terms)
    on_dev = lambda off: torch.from_numpy(off.view(np.int64)).to(dev)                                     # noqa: E731
    first = lambda r: r[0] if isinstance(r, tuple) else r                                                 # noqa: E731

    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "terms_per_call": terms,
           "method": "the legs alternate round by round; median of the timed rounds, spread = max - min; every leg on device tensors, "
                     "timed to the end of a device synchronise; a leg is ahead only where the medians differ by more than the two "
                     "spreads together",
           "legs": {"segmented": "d377_batch_segmented_msm_resident, the caller's offsets_dev",
                    "long": "d377_batch_long_msm_resident on the same buffers (equal lengths)",
                    "ragged": "d377_batch_ragged_msm_resident, window_bits = 0, the same buffers and offsets_dev",
                    "padded": "d377_batch_long_msm_indexed_resident over the points as the pool, every sum padded to the longest with -1",
                    "buckets": "d377_batch_bucket_msm_resident, window_bits = 0 (equal lengths)"},
           "equal_lengths": [], "skewed": None, "crossover": None}

    # ---- (a)
    for en, m in EQUAL:
        en = max(1, en >> a.scale)
        eoff = (np.arange(en + 1, dtype=np.uint64) * np.uint64(m)).astype(np.uint64)
        eoff_dev = on_dev(eoff)
        p, s = pts[:en * m], k[:en * m]
        legs = [("segmented", lambda: ctx.msm_segmented(p, s, eoff, offsets_dev=eoff_dev)), ("long", lambda: ctx.msm_long(p, s, m))]
        times, out = timed(legs, a.warmup, a.reps)
        assert (first(out["segmented"]).cpu() == first(out["long"]).cpu()).all(), (en, m)
        case = {"n": en, "m": m, "plan": ctx.msm_segmented_plan(eoff), "encodings_equal": True,
                "segmented": summary(times["segmented"]), "long": summary(times["long"])}
        case["segmented_minus_long_ms"] = round(case["segmented"]["median_ms"] - case["long"]["median_ms"], 3)
        case["verdict"] = verdict(case["segmented"], case["long"])
        rec["equal_lengths"].append(case)
        print(json.dumps(case), flush=True)

    # ---- (b)
    lengths = skewed(terms, 2, 2048)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    off_dev = on_dev(off)
    n, longest = len(lengths), max(lengths)
    idx = np.full((n, longest), -1, np.int32)
    for i, m in enumerate(lengths):
        idx[i, :m] = np.arange(int(off[i]), int(off[i + 1]))
    didx = torch.from_numpy(idx).to(dev)
    pk = k[torch.from_numpy(np.maximum(idx, 0).astype(np.int64).reshape(-1)).to(dev)].contiguous()   # (an absent term's scalar is not used)
    legs = [("segmented", lambda: ctx.msm_segmented(pts, k, off, offsets_dev=off_dev)),
            ("ragged", lambda: ctx.msm_ragged(pts, k, off, offsets_dev=off_dev)),
            ("padded", lambda: ctx.msm_long_indexed(pts, didx, pk, longest, check_indices=False))]
    times, out = timed(legs, a.warmup, a.reps)
    ref = first(out["segmented"]).cpu()
    equal = {name: bool((first(o).cpu().reshape(ref.shape) == ref).all()) for name, o in out.items()}
    assert all(equal.values()), equal
    case = {"n": n, "terms": terms, "lengths": "%d .. %d doubling, repeating" % (min(lengths), longest), "mean_length": -(-terms // n),
            "plan": ctx.msm_segmented_plan(off), "ragged_plan": ctx.msm_ragged_plan(off), "padded_terms": n * longest, "encodings_equal": equal}
    for name, _ in legs:
        case[name] = summary(times[name])
    case["verdict_against_ragged"] = verdict(case["segmented"], case["ragged"])
    case["verdict_against_padded"] = verdict(case["segmented"], case["padded"])
    rec["skewed"] = case
    print(json.dumps(case), flush=True)

    # ---- (c)
    sweep, constant = [], None
    for m in SWEEP:
        en = max(1, terms // m)
        p, s = pts[:en * m], k[:en * m]
        legs = [("long", lambda: ctx.msm_long(p, s, m)), ("buckets", lambda: ctx.msm_buckets(p, s, m))]
        times, out = timed(legs, a.warmup, a.reps)
        assert (first(out["long"]).cpu() == first(out["buckets"]).cpu()).all(), m
        row = {"n": en, "m": m, "long": summary(times["long"]), "buckets": summary(times["buckets"])}
        row["buckets_ahead"] = verdict(row["buckets"], row["long"]) == "use this call"
        if row["buckets_ahead"] and constant is None:
            constant = m
        sweep.append(row)
        print(json.dumps(row), flush=True)
    in_force = next((m for m in range(1, 1 << 13) if ctx.msm_segmented_plan([0, m])["advised_route"] == "buckets"), None)
    rec["crossover"] = {"sweep": sweep, "smallest_length_with_buckets_ahead": constant,
                        "case": "established by this sweep" if constant is not None else "none established: 1024, the point measured before, is kept",
                        "constant_in_force": in_force}
    print(json.dumps(rec["crossover"]), flush=True)
    if not a.scale:
        with open(a.out or os.path.join(root, "profiles", "segmented_sums_bench.json"), "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
