#!/usr/bin/env python3
"""The pooled DeepFM step of the second-order table (forward + backward), fused against composed, on the full Criteo-sized table.

Per shape (B, F, d) three variants are timed in ONE process, alternating, `--reps` windows each:

  (a) fused      ha_gather_fm_f32ids without rows (S and 0.5 * (S*S - Q)), then ha_sgd_apply_fm_bags: no [n, d] tensor
  (b) composed   ha_gather_fm_f32ids with rows, g_sum expanded to [n, d] (the gather kernel over g_sum, as
                 IndexedSlices.expanded_values does it), ha_fm_grad_rows in place, ha_sgd_apply_finished -- the same bits
  (c) bound      ha_sgd_apply_bags alone on g_sum: it moves the same table rows and does none of the FM arithmetic (and no
                 forward) -- a lower bound for (a)'s apply, not a variant of the step

The index plan of every batch (sort + finish) is built before the windows: all three consume the same plan.  A window is
`--iters` steps over `--distinct` different batches (herald_amd.synth.criteo_batch), captured into one device graph so that the
device runs them back to back, between two device events; the figure of a window is its time / iters.  Every variant is warmed
up before anything is timed.  Reported per variant: median, minimum and maximum over the windows.  There is no threshold: where
(a) is not faster than (b) outside the spread the line says so.

Kernel times: run under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/fm_pooled_bench.py --no-graph --reps 1 ...`
(the kernels are bag_fm_kernel, fm_apply_kernel, gather_vec4_kernel, fm_grad_rows_kernel, apply_kernel, apply_bags_kernel).
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
from fm_bench import compare                         # noqa: E402


def summarise(times):
    return {name: {"median_us": float(np.median(ts)), "min_us": float(min(ts)), "max_us": float(max(ts)), "windows": len(ts)}
            for name, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x26x128,256x26x512,4096x26x128", help="B x F x d, comma separated")
    ap.add_argument("--rows", type=int, default=synth.CRITEO_ROWS)
    ap.add_argument("--reps", type=int, default=15, help="timed windows per variant")
    ap.add_argument("--iters", type=int, default=200, help="steps per window")
    ap.add_argument("--distinct", type=int, default=32, help="different batches cycled through a window")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--no-graph", action="store_true", help="plain launches instead of one device graph per window")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fm_pooled_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
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
        longest = int(max(np.unique(h, return_counts=True)[1].max() for h in host))
        ids = [torch.from_numpy(h).to(dev) for h in host]
        nd = len(ids)
        plans = [ops.IndexPlan(n, dev).sort(t.reshape(-1)).finish() for t in ids]
        gen = torch.Generator(device=dev)
        gen.manual_seed(456)
        g_sum = torch.randn((B, d), dtype=torch.float32, device=dev, generator=gen) * 0.1
        g_fm = torch.randn((B, d), dtype=torch.float32, device=dev, generator=gen) * 0.1
        total = torch.empty((B, d), dtype=torch.float32, device=dev)
        fm = torch.empty((B, d), dtype=torch.float32, device=dev)
        rows_out = torch.empty((B, F, d), dtype=torch.float32, device=dev)
        g_rows = torch.empty((B, F, d), dtype=torch.float32, device=dev)
        which = torch.arange(n, dtype=torch.int64, device=dev) // F
        torch.cuda.synchronize(dev)

        def fused(i):
            ops.embedding_lookup_fm(table, ids[i % nd], sum_out=total, fm_out=fm, want_rows=False)
            ops.sgd_apply_fm_bags(table, plans[i % nd], g_sum, g_fm, total, args.lr, bag=F)

        def composed(i):
            ops.embedding_lookup_fm(table, ids[i % nd], rows_out=rows_out, sum_out=total, fm_out=fm)
            ops.embedding_lookup(g_sum, which, out=g_rows)
            ops.fm_grad_rows(g_rows, rows_out, total, g_fm, bag=F, out=g_rows)
            ops.sgd_apply(table, plans[i % nd], g_rows, args.lr, finished=True)

        def bound(i):
            ops.sgd_apply_bags(table, plans[i % nd], g_sum, args.lr, bag=F)

        res = summarise(time_variants({"fused": fused, "composed": composed, "bound": bound}, args.reps, args.iters,
                                      not args.no_graph, dev))
        entry = {"n": n, "mean_unique": U, "longest_run": longest, "variants": res,
                 "comparisons": {"fused vs composed": compare(res, "fused", "composed"),
                                 "fused vs bound": compare(res, "fused", "bound")}}
        results["shapes"]["%dx%dx%d" % (B, F, d)] = entry
        print("== B=%d F=%d d=%d  n=%d  mean unique %.0f  longest run %d" % (B, F, d, n, U, longest))
        for name, r in res.items():
            print("  %-9s median %8.2f us  [%7.2f .. %7.2f]  over %d windows" % (name, r["median_us"], r["min_us"], r["max_us"],
                                                                                r["windows"]))
        for name, v in entry["comparisons"].items():
            print("  %-18s %s is %s  (difference %+.2f us, spread %.2f us)" % (name, v["a"], v["a_is"], v["a_minus_b_us"],
                                                                              v["spread_us"]))
        sys.stdout.flush()
        del plans
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
