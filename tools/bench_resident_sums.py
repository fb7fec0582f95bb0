#!/usr/bin/env python3
"""The resident forms of the sums over registered bases against the host-pointer forms of the same sums (d377_batch_*_resident
against d377_batch_fixed_msm, d377_batch_fixed_msm_indexed, d377_batch_msm_mixed), in one process on one device:
  (a) the resident call: torch tensors that already live on the device, torch's current stream, outputs allocated there;
      the indexed and mixed sums with check_indices=False, so the call reads nothing back -- wall-clock from the call to the end
      of a device synchronise;
  (b) the host-pointer call on numpy arrays of the same values (it returns synchronised): the reference, unchanged code.
The two legs ALTERNATE: after the warm-up rounds every round times (a) and then (b); the median of the rounds is reported with
each leg's min-to-max spread, and the Encodings of the two legs must be equal.  "a_ahead" / "b_ahead" are true where one median
is ahead of the other by more than the two spreads together; anything else is a tie.
For the indexed sums the verdict kernel is also timed alone (device events around d377_check_base_index_resident, median of the
same number of rounds) and reported as a share of the resident call.
    python tools/bench_resident_sums.py [--reps 5] [--warmup 2]     ->  profiles/resident_sums_bench.json, one JSON line per case
    python tools/bench_resident_sums.py --scale 10                   (every n divided by 2^10, printed and not written)"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import decaf377_amd as d

# (kind, n, shape): the shapes README.md quotes for the host path
CASES = [("dense", 1 << 20, {"bases": 1, "bits": 18}),
         ("dense", 1 << 20, {"bases": 3, "bits": 16}),
         ("indexed", 1 << 20, {"bases": 64, "bits": 16, "t": 2}),
         ("mixed", 1 << 20, {"bases": 1, "bits": 16, "t": 1, "v": 1}),
         ("mixed", 1 << 12, {"bases": 1, "bits": 16, "t": 1, "v": 1})]


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
            "spread_ms": round(max(ts) - min(ts), 3), "reps": len(ts)}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=int, default=0, help="divide every n by 2^SCALE (a rehearsal: printed and not written)")
    ap.add_argument("--out", default=os.path.join(root, "profiles", "resident_sums_bench.json"))
    a = ap.parse_args()
    ctx = d.Context([0], comb_lazy=True)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(12)
    rnd = lambda rows: torch.randint(0, 256, (rows, 32), dtype=torch.uint8, device=dev, generator=gen)
    points = lambda rows: ctx.decompress(ctx.encode_to_curve(rnd(rows)))[0]
    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    rec = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
           "method": "legs alternate round by round; median of the timed rounds, spread = max - min; a tie unless one median is "
                     "ahead by more than both spreads together",
           "legs": {"a": "resident: torch tensors on the device, wall-clock to the end of a device synchronise",
                    "b": "host pointers: numpy arrays, the call returns synchronised"},
           "cases": []}
    for kind, n, shape in CASES:
        n = max(1, n >> a.scale)
        fb = ctx.fixed_bases(u64(points(shape["bases"])), comb_bits=shape["bits"])
        if kind == "dense":
            k = rnd(n * shape["bases"])
            hk = k.cpu().numpy()
            resident = lambda: fb.msm(k)
            host = lambda: fb.msm(hk)
        else:
            t = shape["t"]
            idx = torch.randint(0, shape["bases"], (n, t), dtype=torch.int32, device=dev, generator=gen)
            fk = rnd(n * t)
            hidx, hfk = idx.cpu().numpy(), fk.cpu().numpy()
            if kind == "indexed":
                resident = lambda: fb.msm_indexed(idx, fk, check_indices=False)[0]
                host = lambda: fb.msm_indexed(hidx, hfk)
            else:
                v = shape["v"]
                P, vk = points(n * v), rnd(n * v)
                hP, hvk = u64(P), vk.cpu().numpy()
                resident = lambda: fb.msm_mixed(idx, fk, P, vk, check_indices=False)[0]
                host = lambda: fb.msm_mixed(hidx, hfk, hP, hvk)
        torch.cuda.synchronize()
        times = {"a": [], "b": []}
        out = {}
        for r in range(a.warmup + a.reps):
            for name, fn in (("a", resident), ("b", host)):
                t0 = time.perf_counter()
                out[name] = fn()
                if name == "a":
                    torch.cuda.synchronize()
                if r >= a.warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        assert (out["a"].cpu().numpy() == out["b"]).all(), (kind, n, shape)
        ta, tb = summary(times["a"]), summary(times["b"])
        case = dict(kind=kind, n=n, **shape)
        case.update({"a_resident": ta, "b_host": tb, "encodings_equal": True, "b_over_a": round(tb["median_ms"] / ta["median_ms"], 2),
                     "a_ahead": bool(tb["median_ms"] - ta["median_ms"] > ta["spread_ms"] + tb["spread_ms"]),
                     "b_ahead": bool(ta["median_ms"] - tb["median_ms"] > ta["spread_ms"] + tb["spread_ms"])})
        if kind == "indexed":                                    # the verdict kernel alone, by device events
            verdict = torch.zeros((2,), dtype=torch.int64, device=dev)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            ev = []
            for r in range(a.warmup + a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                d._native.check(ctx._lib.d377_check_base_index_resident(ctx._h, 0, stream, fb._h, ctypes.c_void_p(idx.data_ptr()),
                                                                        ctypes.c_size_t(idx.numel()), ctypes.c_void_p(verdict.data_ptr())))
                e1.record()
                torch.cuda.synchronize()
                if r >= a.warmup:
                    ev.append(e0.elapsed_time(e1))
            assert verdict.cpu().tolist() == [0, -1]
            case["verdict_kernel"] = summary(ev)
            case["verdict_share_of_a"] = round(case["verdict_kernel"]["median_ms"] / ta["median_ms"], 4)
        fb.close()
        rec["cases"].append(case)
        print(json.dumps(case), flush=True)
    if not a.scale:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
