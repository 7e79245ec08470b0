#!/usr/bin/env python3
"""FM-pooled lookup and its gradient (the DeepFM models) against the per-occurrence lookup plus the PyTorch passes they replace,
on the full Criteo-sized table.

Per shape (B, F, d) the variants below are timed in ONE process, alternating, `--reps` windows each:

  forward   fused             ha_gather_fm_f32ids: rows, S and 0.5 * (S*S - Q) in one pass
            gather+torch      ha_gather_f32ids, then S = rows.sum(1), Q = (rows * rows).sum(1), 0.5 * (S*S - Q) in PyTorch
            gather            ha_gather_f32ids alone (what any model that wants the rows pays)
  backward  fused             ha_fm_grad_rows, in place over the rows' gradient
            torch             g_rows + (g_fm * S)[:, None, :] - g_fm[:, None, :] * rows in PyTorch (out=-less: its temporaries)
  first     sum               the width-1 sum-pooled lookup of the first-order table (ha_gather_sum_f32ids, width 1)
            bags              its sparse SGD from the [B, 1] gradient (ha_sgd_apply_bags; the plan is built before the window)

A window is `--iters` calls over `--distinct` different batches (herald_amd.synth.criteo_batch), captured into one device graph
so that the device runs them back to back, between two device events; the figure of a window is its time / iters.  Every
variant is warmed up before anything is timed.  Reported per variant: median, minimum and maximum over the windows, and the
bytes the algorithm needs (computed from the shapes, below) over the median.  There is no threshold: where a fused form is
slower than the unfused one the line says so.

Kernel times: run under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/fm_bench.py --no-graph --reps 1 ...` (the
kernels are bag_fm_kernel, fm_grad_rows_kernel, gather_vec4_kernel, bag_sum_kernel, apply_bags_kernel).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from herald_amd import ops, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bag_bench import init_table, time_variants      # noqa: E402  (the same table and the same windows)


def forward_bytes(B, F, d):
    n = B * F
    rows = n * 4 * d
    return {"fused": n * 4 + 2 * rows + 2 * B * 4 * d,             # ids, rows read once and written once, S and fm
            "gather": n * 4 + 2 * rows,
            # the gather, then sum (read rows), square (read rows, write a temporary), sum (read it), and the [B, d] passes
            "gather+torch": n * 4 + 2 * rows + rows + 2 * rows + rows + 8 * B * 4 * d}


def backward_bytes(B, F, d):
    n = B * F
    rows = n * 4 * d
    return {"fused": 3 * rows + 2 * B * 4 * d,                     # g_rows and rows read, the gradient written; S and g_fm
            # g_fm * S; g_fm[:, None] * rows (read rows, write a temporary); g_rows + ... (a temporary); the subtraction
            "torch": 3 * B * 4 * d + 2 * rows + 2 * rows + 3 * rows}


def first_bytes(B, F, U):
    n = B * F
    return {"sum": n * 8 + B * 4, "bags": n * 8 + B * 4 + U * 8}


def summarise(times, nbytes):
    out = {}
    for name, ts in times.items():
        med = float(np.median(ts))
        out[name] = {"median_us": med, "min_us": float(min(ts)), "max_us": float(max(ts)), "windows": len(ts),
                     "bytes": int(nbytes[name]), "GBps_at_median": nbytes[name] / med * 1e-3}
    return out


def compare(res, a, b):
    """a against b: the difference of the medians beside the larger of the two window spreads."""
    spread = max(res[a]["max_us"] - res[a]["min_us"], res[b]["max_us"] - res[b]["min_us"])
    diff = res[a]["median_us"] - res[b]["median_us"]
    word = "faster" if diff < -spread else ("SLOWER" if diff > spread else "equal within the spread")
    return {"a": a, "b": b, "a_minus_b_us": diff, "spread_us": spread, "a_is": word}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x26x128,256x26x512,4096x26x128", help="B x F x d, comma separated")
    ap.add_argument("--rows", type=int, default=synth.CRITEO_ROWS)
    ap.add_argument("--reps", type=int, default=15, help="timed windows per variant")
    ap.add_argument("--iters", type=int, default=200, help="calls per window")
    ap.add_argument("--distinct", type=int, default=32, help="different batches cycled through a window")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--no-graph", action="store_true", help="plain launches instead of one device graph per window")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fm_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    results = {"rows": args.rows, "reps": args.reps, "iters": args.iters, "distinct": args.distinct,
               "graph": not args.no_graph, "device": torch.cuda.get_device_name(dev), "shapes": {}}
    first_table = init_table(args.rows, 1, dev, seed=321)
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
        gen = torch.Generator(device=dev)
        gen.manual_seed(456)
        # ---- forward
        rows_out = torch.empty((B, F, d), dtype=torch.float32, device=dev)
        total = torch.empty((B, d), dtype=torch.float32, device=dev)
        fm = torch.empty((B, d), dtype=torch.float32, device=dev)

        def fused(i):
            ops.embedding_lookup_fm(table, ids[i % nd], rows_out=rows_out, sum_out=total, fm_out=fm)

        def gather(i):
            ops.embedding_lookup(table, ids[i % nd], out=rows_out)

        def gather_torch(i):
            ops.embedding_lookup(table, ids[i % nd], out=rows_out)
            s = rows_out.sum(1)
            q = (rows_out * rows_out).sum(1)
            torch.mul(s * s - q, 0.5, out=fm)

        fres = summarise(time_variants({"fused": fused, "gather+torch": gather_torch, "gather": gather}, args.reps, args.iters,
                                       not args.no_graph, dev), forward_bytes(B, F, d))
        # ---- backward (the forward's outputs of the last batch stand in for every batch: the traffic is the same)
        fused(0)
        g_rows = torch.randn((B, F, d), dtype=torch.float32, device=dev, generator=gen)
        g_fm = torch.randn((B, d), dtype=torch.float32, device=dev, generator=gen)
        g_work = g_rows.clone()

        def grad_fused(i):
            ops.fm_grad_rows(g_work, rows_out, total, g_fm, bag=F, out=g_work)

        def grad_torch(i):
            return g_rows + (g_fm * total)[:, None, :] - g_fm[:, None, :] * rows_out

        bres = summarise(time_variants({"fused": grad_fused, "torch": grad_torch}, args.reps, args.iters, not args.no_graph,
                                       dev), backward_bytes(B, F, d))
        # ---- the first-order table: width 1
        pooled1 = torch.empty((B, 1), dtype=torch.float32, device=dev)
        plans = [ops.IndexPlan(n, dev).sort(t.reshape(-1)) for t in ids]
        g1 = torch.randn((B, 1), dtype=torch.float32, device=dev, generator=gen)

        def first_sum(i):
            ops.embedding_lookup_sum(first_table, ids[i % nd], out=pooled1)

        def first_bags(i):
            ops.sgd_apply_bags(first_table, plans[i % nd], g1, args.lr, bag=F)

        ores = summarise(time_variants({"sum": first_sum, "bags": first_bags}, args.reps, args.iters, not args.no_graph, dev),
                         first_bytes(B, F, U))
        entry = {"n": n, "mean_unique": U, "forward": fres, "backward": bres, "first": ores,
                 "comparisons": {"forward fused vs gather+torch": compare(fres, "fused", "gather+torch"),
                                 "backward fused vs torch": compare(bres, "fused", "torch")}}
        results["shapes"]["%dx%dx%d" % (B, F, d)] = entry
        print("== B=%d F=%d d=%d  n=%d  mean unique %.0f" % (B, F, d, n, U))
        for side in ("forward", "backward", "first"):
            for name, r in entry[side].items():
                print("  %-8s %-13s median %8.2f us  [%7.2f .. %7.2f]  %7.2f MB  %7.1f GB/s" % (
                    side, name, r["median_us"], r["min_us"], r["max_us"], r["bytes"] / 1e6, r["GBps_at_median"]))
        for name, v in entry["comparisons"].items():
            print("  %-32s fused is %s  (difference %+.2f us, spread %.2f us)" % (name, v["a_is"], v["a_minus_b_us"],
                                                                                 v["spread_us"]))
        sys.stdout.flush()
        del plans
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
