#!/usr/bin/env python3
"""d377_batch_msm_long against what a caller had before it: n independent m-term sums
  (a) as ONE call of d377_batch_msm_long,
  (b) as n calls of d377_msm,
  (c) as the composition: d377_batch_msm_small on groups of 8 with Element records out, ceil(log2 g) rounds of d377_batch_add,
      one d377_batch_compress.
All three on host (numpy) arrays -- the new call is host-pointer only -- in one process on one device, wall-clock per call
(every host-pointer call returns synchronised), warm-up calls before the timed ones, the median of the timed ones reported.
Leg (b) is timed on at most --msm-calls sums and scaled to n (its calls are independent and equally long); the record says so.
Every case carries its verdict, median against median: "a_no_slower_than_b", "a_no_slower_than_c", and the record's "a_loses"
lists every (n, m, leg) at which the new call is the slower one -- at (1, 4096), one long sum, d377_msm is expected there.
    python tools/batch_msm_long_bench.py [--reps 5] [--warmup 2]   ->  profiles/batch_msm_long_bench.json, one JSON line per shape
    rocprofv3 --kernel-trace --stats -- python tools/batch_msm_long_bench.py --only 256,4096   (the kernels' own times of one shape)"""
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

SHAPES = [(1 << 16, 16), (1 << 12, 256), (1 << 8, 4096), (1, 4096)]


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--msm-calls", type=int, default=128, help="leg (b): time at most this many d377_msm calls and scale to n")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "batch_msm_long_bench.json"))
    ap.add_argument("--only", default=None, help="n,m: that one shape (m a multiple of 8), printed and not written -- for a kernel trace of one case")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in a.only.split(","))] if a.only else SHAPES
    ctx = d.Context([0], comb_lazy=True)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(11)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "path": "host (numpy)",
           "legs": {"a": "d377_batch_msm_long", "b": "n x d377_msm", "c": "d377_batch_msm_small (groups of 8) + rounds of d377_batch_add + d377_batch_compress"},
           "cases": [], "a_loses": []}
    for n, m in shapes:
        terms = n * m
        r0 = torch.randint(0, 256, (terms, 32), dtype=torch.uint8, device=dev, generator=gen)
        P = ctx.decompress(ctx.encode_to_curve(r0))[0].cpu().numpy().view(np.uint64)
        k = torch.randint(0, 256, (terms, 32), dtype=torch.uint8, device=dev, generator=gen).cpu().numpy()
        assert m % 8 == 0
        g = m // 8

        def long_call():
            return ctx.msm_long(P, k, m)

        def composed():
            _, x = ctx.msm_small(P, k, 8, elements=True)            # [n g, 16]: the groups of sum s are records s g .. s g + g - 1
            c = g
            while c > 1:                                             # c is a power of two at these shapes
                x = x.reshape(n, c, 16)
                x = ctx.add(np.ascontiguousarray(x[:, 0::2]).reshape(-1, 16), np.ascontiguousarray(x[:, 1::2]).reshape(-1, 16))
                c //= 2
            return ctx.compress(x)

        calls = min(n, a.msm_calls)

        def msm_calls():
            return [ctx.msm(P[s * m:(s + 1) * m], k[s * m:(s + 1) * m])[0] for s in range(calls)]

        got = long_call()
        assert (got == composed()).all(), (n, m)
        assert (got[:calls] == np.stack(msm_calls())).all(), (n, m)
        ta = timed(long_call, a.warmup, a.reps)
        tc = timed(composed, a.warmup, a.reps)
        tb = timed(msm_calls, 1, max(2, a.reps // 2))
        scale = n / calls
        b_ms = tb["median_ms"] * scale
        case = {"n": n, "m": m, "terms": terms, "a_msm_long": ta, "c_composition": tc,
                "b_msm_per_sum": {"timed_calls": calls, "timed": tb, "scaled_to_n_ms": round(tb["median_ms"] * scale, 3), "extrapolated": calls != n},
                "b_over_a": round(tb["median_ms"] * scale / ta["median_ms"], 2), "c_over_a": round(tc["median_ms"] / ta["median_ms"], 2),
                "a_terms_per_sec": round(terms / (ta["median_ms"] * 1e-3)),
                "many_sums": n > 1, "a_no_slower_than_b": ta["median_ms"] <= b_ms, "a_no_slower_than_c": ta["median_ms"] <= tc["median_ms"]}
        rec["cases"].append(case)
        rec["a_loses"] += [{"n": n, "m": m, "to": leg} for leg, ok in (("b", case["a_no_slower_than_b"]), ("c", case["a_no_slower_than_c"])) if not ok]
        print(json.dumps(case), flush=True)
    for lost in rec["a_loses"]:
        print("d377_batch_msm_long is SLOWER than leg (%s) at (n, m) = (%d, %d)" % (lost["to"], lost["n"], lost["m"]), flush=True)
    if not a.only:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
