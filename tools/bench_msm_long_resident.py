#!/usr/bin/env python3
"""The long sums on device buffers and over a pool of points (include/decaf377_amd_long_sums.h) against the forms they stand
beside, in one process on one device, 2^20 terms per call at (n, m) = (2^16, 16), (2^12, 256) and (2^8, 4096).  Three pairs of
legs per shape:
  resident          (a) d377_batch_long_msm_resident on torch tensors that already live on the device, torch's current stream,
                    wall-clock from the call to the end of a device synchronise; (b) d377_batch_msm_long on numpy arrays of the
                    same values (it returns synchronised)
  indexed_host      (a) d377_batch_long_msm_indexed on numpy arrays, a pool of m points shared by all sums (36 bytes per term
                    cross the bus, and the pool once); (b) d377_batch_msm_long on the materialised n x m records (160 bytes)
  indexed_resident  (a) d377_batch_long_msm_indexed_resident (check_indices=False: nothing is read back) against (b) the plain
                    resident call on the materialised array, both to the end of a device synchronise: what the gather costs
The two legs of a pair ALTERNATE: after the warm-up rounds every round times (a) and then (b); the median of the rounds is
reported with each leg's min-to-max spread, and the Encodings of the two legs must be equal.  "a_ahead" / "b_ahead" are true
where one median is ahead of the other by more than the two spreads together; anything else is not established.
    python tools/bench_msm_long_resident.py [--reps 5] [--warmup 2]   ->  profiles/msm_long_resident_bench.json, one JSON line per pair
    python tools/bench_msm_long_resident.py --scale 8                  (every n divided by 2^8, printed and not written)"""
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

SHAPES = [(1 << 16, 16), (1 << 12, 256), (1 << 8, 4096)]


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
            "spread_ms": round(max(ts) - min(ts), 3), "reps": len(ts)}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=0, help="divide every n by 2^SCALE (a rehearsal: printed and not written)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "msm_long_resident_bench.json"))
    a = ap.parse_args()
    ctx = d.Context([0], comb_lazy=True)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(12)
    rnd = lambda rows: torch.randint(0, 256, (rows, 32), dtype=torch.uint8, device=dev, generator=gen)
    points = lambda rows: ctx.decompress(ctx.encode_to_curve(rnd(rows)))[0]
    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "method": "the legs of a pair alternate round by round; median of the timed rounds, spread = max - min; not established "
                     "unless one median is ahead by more than both spreads together",
           "pairs": {"resident": "a: resident call on device tensors, to the end of a device synchronise; b: host pointers, numpy arrays",
                     "indexed_host": "a: indexed host form, a pool of m points shared by all sums; b: host form on the materialised array",
                     "indexed_resident": "a: indexed resident form; b: plain resident form on the materialised array; both to the end "
                                         "of a device synchronise"},
           "cases": []}
    for n, m in SHAPES:
        n = max(1, n >> a.scale)
        pool = points(m)
        idx = torch.randint(0, m, (n, m), dtype=torch.int32, device=dev, generator=gen)
        k = rnd(n * m)
        pts = pool[idx.reshape(-1).long()].contiguous()           # the materialised n x m records
        hpool, hidx, hk, hpts = u64(pool), idx.cpu().numpy(), k.cpu().numpy(), u64(pts)
        pairs = [("resident", lambda: ctx.msm_long(pts, k, m), lambda: ctx.msm_long(hpts, hk, m)),
                 ("indexed_host", lambda: ctx.msm_long_indexed(hpool, hidx, hk, m), lambda: ctx.msm_long(hpts, hk, m)),
                 ("indexed_resident", lambda: ctx.msm_long_indexed(pool, idx, k, m, check_indices=False)[0], lambda: ctx.msm_long(pts, k, m))]
        for pair, leg_a, leg_b in pairs:
            torch.cuda.synchronize()
            times = {"a": [], "b": []}
            out = {}
            for r in range(a.warmup + a.reps):
                for name, fn in (("a", leg_a), ("b", leg_b)):
                    t0 = time.perf_counter()
                    out[name] = fn()
                    torch.cuda.synchronize()                     # (a host-pointer leg has returned synchronised: nothing to wait for)
                    if r >= a.warmup:
                        times[name].append((time.perf_counter() - t0) * 1e3)
            host = lambda o: o.cpu().numpy() if hasattr(o, "cpu") else o
            assert (host(out["a"]) == host(out["b"])).all(), (pair, n, m)
            ta, tb = summary(times["a"]), summary(times["b"])
            case = {"pair": pair, "n": n, "m": m, "a": ta, "b": tb, "encodings_equal": True,
                    "b_over_a": round(tb["median_ms"] / ta["median_ms"], 2),
                    "a_ahead": bool(tb["median_ms"] - ta["median_ms"] > ta["spread_ms"] + tb["spread_ms"]),
                    "b_ahead": bool(ta["median_ms"] - tb["median_ms"] > ta["spread_ms"] + tb["spread_ms"])}
            rec["cases"].append(case)
            print(json.dumps(case), flush=True)
    if not a.scale:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
