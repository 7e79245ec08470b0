#!/usr/bin/env python3
"""Sum-pooled lookup and bag apply against the per-occurrence calls they replace, on the full Criteo-sized table.

Per shape (B, F, d) the variants below are timed in ONE process, alternating, `--reps` windows each:

  forward   fused             ha_gather_sum_f32ids, slice width chosen by the library
            fused/64|128|256  the same with the column slice of a wave forced (ha_debug_bag_slice): the slice-width A/B
            gather            ha_gather_f32ids alone (the same rows read, 26 times the output written)
            gather+sum        ha_gather_f32ids followed by torch.sum(1)
  backward  bags              ha_sgd_apply_bags, fixed bags (source row = occurrence / F in registers)
            mapped            ha_apply_mapped with valmap = bag_of (the same rows through an index map)
            expanded          ha_sgd_apply on the gradient expanded to [n, d]
  (plans are built before the timed windows)

A window is `--iters` calls over `--distinct` different batches (herald_amd.synth.criteo_batch), captured into one device graph
so that the device runs them back to back, between two device events; the figure of a window is its time / iters.  Every
variant is warmed up before anything is timed.  Reported per variant: median, minimum and maximum over the windows, and the
bytes the algorithm needs (computed from the shapes and the batches' unique counts, below) over the median.

The two conditions of the feature are evaluated at the end: fused <= gather and bags <= expanded, where a difference within
the larger of the two variants' own window spreads counts as equal.

Kernel times: run under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bag_bench.py --no-graph --reps 1 ...` (the
kernels are bag_sum_kernel, gather_vec4_kernel, apply_bags_kernel, apply_mapped_kernel, apply_kernel).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from herald_amd import _lib, ops, synth


def init_table(rows, width, dev, seed=123):
    """The table as bench.py builds it: N(0, 0.01), filled on the device in chunks."""
    t = torch.empty((rows, width), dtype=torch.float32, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    chunk = 1 << 20
    for s in range(0, rows, chunk):
        t[s:s + chunk].normal_(0.0, 0.01, generator=g)
    return t


def forward_bytes(B, F, d):
    n = B * F
    return {"fused": n * (4 * d + 4) + B * 4 * d,
            "gather": n * (4 * d + 4) + n * 4 * d,
            "gather+sum": n * (4 * d + 4) + n * 4 * d + n * 4 * d + B * 4 * d}


def backward_bytes(B, F, d, U):
    n = B * F
    table = U * 8 * d                                   # every unique row read and written once
    return {"bags": n * 8 + B * 4 * d + table,          # sorted keys + occurrence indices, the distinct gradient rows
            "mapped": n * 12 + B * 4 * d + table,       # ... and the bag map
            "expanded": n * 8 + n * 4 * d + table}


def time_variants(variants, reps, iters, use_graph, dev):
    """variants: {name: f(i)}; -> {name: [microseconds per call, one per window]}."""
    runs = {}
    for name, f in variants.items():
        for i in range(min(iters, 8)):                  # warm-up: code objects, allocator
            f(i)
        torch.cuda.synchronize(dev)
        if use_graph:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for i in range(iters):
                    f(i)
            runs[name] = g.replay
            g.replay()                                  # warm-up of the graph itself
        else:
            runs[name] = (lambda f=f: [f(i) for i in range(iters)])
    torch.cuda.synchronize(dev)
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, run in runs.items():                  # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / iters)
    return times


def summarise(times, nbytes):
    out = {}
    for name, ts in times.items():
        med = float(np.median(ts))
        key = name.split("/")[0]
        out[name] = {"median_us": med, "min_us": float(min(ts)), "max_us": float(max(ts)), "windows": len(ts),
                     "bytes": int(nbytes[key]), "GBps_at_median": nbytes[key] / med * 1e-3}
    return out


def verdict(res, a, b):
    """a <= b, a difference within the larger of the two spreads counting as equal."""
    spread = max(res[a]["max_us"] - res[a]["min_us"], res[b]["max_us"] - res[b]["min_us"])
    diff = res[a]["median_us"] - res[b]["median_us"]
    return {"a": a, "b": b, "a_minus_b_us": diff, "spread_us": spread, "met": bool(diff <= spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x26x512,256x26x128,4096x26x128", help="B x F x d, comma separated")
    ap.add_argument("--rows", type=int, default=synth.CRITEO_ROWS)
    ap.add_argument("--reps", type=int, default=15, help="timed windows per variant")
    ap.add_argument("--iters", type=int, default=200, help="calls per window")
    ap.add_argument("--distinct", type=int, default=32, help="different batches cycled through a window")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--no-graph", action="store_true", help="plain launches instead of one device graph per window")
    ap.add_argument("--no-slices", action="store_true", help="skip the slice-width A/B")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bag_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    L = _lib.load()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    results = {"rows": args.rows, "reps": args.reps, "iters": args.iters, "distinct": args.distinct,
               "graph": not args.no_graph, "device": torch.cuda.get_device_name(dev), "shapes": {}}
    table, table_d = None, None
    for (B, F, d) in shapes:
        if table_d != d:
            table = None
            torch.cuda.empty_cache()
            table, table_d = init_table(args.rows, d, dev), d
        n = B * F
        host = [synth.as_f32_ids(synth.criteo_batch(B, step=s, rows=args.rows, nfields=F)) for s in range(args.distinct)]
        U = float(np.mean([np.unique(h).size for h in host]))
        ids = [torch.from_numpy(h).to(dev) for h in host]
        nd = len(ids)
        # ---- forward
        pooled = torch.empty((B, d), dtype=torch.float32, device=dev)
        rows_out = torch.empty((B, F, d), dtype=torch.float32, device=dev)

        def fused(i):
            ops.embedding_lookup_sum(table, ids[i % nd], out=pooled)

        def fused_slice(floats):
            def f(i):
                L.ha_debug_bag_slice(floats)
                ops.embedding_lookup_sum(table, ids[i % nd], out=pooled)
                L.ha_debug_bag_slice(0)
            return f

        def gather(i):
            ops.embedding_lookup(table, ids[i % nd], out=rows_out)

        def gather_sum(i):
            ops.embedding_lookup(table, ids[i % nd], out=rows_out)
            torch.sum(rows_out, dim=1, out=pooled)

        fwd = {"fused": fused, "gather": gather, "gather+sum": gather_sum}
        if not args.no_slices and d % 4 == 0:
            for floats in (64, 128, 256):
                fwd["fused/%d" % floats] = fused_slice(floats)
        fres = summarise(time_variants(fwd, args.reps, args.iters, not args.no_graph, dev), forward_bytes(B, F, d))
        # ---- backward (plans prebuilt, untimed)
        plans = [ops.IndexPlan(n, dev).sort(t.reshape(-1)) for t in ids]
        gen = torch.Generator(device=dev)
        gen.manual_seed(456)
        bag_grads = torch.randn((B, d), dtype=torch.float32, device=dev, generator=gen)
        expanded = bag_grads.repeat_interleave(F, 0).contiguous()
        which = (torch.arange(n, device=dev) // F).to(torch.int32)
        vp = ctypes.c_void_p

        def bags(i):
            ops.sgd_apply_bags(table, plans[i % nd], bag_grads, args.lr, bag=F)

        def mapped(i):
            _lib.check(L.ha_apply_mapped(vp(table.data_ptr()), args.rows, d, vp(plans[i % nd].ws.data_ptr()), n,
                                         vp(bag_grads.data_ptr()), ctypes.c_float(args.lr), None, vp(which.data_ptr()), None,
                                         ops._stream_ptr()), "ha_apply_mapped")

        def expand(i):
            ops.sgd_apply(table, plans[i % nd], expanded, args.lr)

        bres = summarise(time_variants({"bags": bags, "mapped": mapped, "expanded": expand}, args.reps, args.iters,
                                       not args.no_graph, dev), backward_bytes(B, F, d, U))
        entry = {"n": n, "mean_unique": U, "forward": fres, "backward": bres,
                 "conditions": {"fused<=gather": verdict(fres, "fused", "gather"),
                                "bags<=expanded": verdict(bres, "bags", "expanded")}}
        results["shapes"]["%dx%dx%d" % (B, F, d)] = entry
        print("== B=%d F=%d d=%d  n=%d  mean unique %.0f" % (B, F, d, n, U))
        for side in ("forward", "backward"):
            for name, r in entry[side].items():
                print("  %-8s %-11s median %8.2f us  [%7.2f .. %7.2f]  %6.2f MB  %7.1f GB/s" % (
                    side, name, r["median_us"], r["min_us"], r["max_us"], r["bytes"] / 1e6, r["GBps_at_median"]))
        for name, v in entry["conditions"].items():
            print("  condition %-15s %s  (difference %+.2f us, spread %.2f us)" % (name, "met" if v["met"] else "MISSED",
                                                                                  v["a_minus_b_us"], v["spread_us"]))
        sys.stdout.flush()
        del plans
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
