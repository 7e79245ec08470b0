#!/usr/bin/env python3
"""AdaGrad / Adam steps from the pooled gradient against the same steps from the expanded one, on the full Criteo-sized table.

Per shape (B, F, d) and optimizer the three variants below are timed in ONE process, alternating, `--reps` windows each:

  bags              ha_sparse_opt_fused_bags_f32ids: plan + fused dedup / optimizer launch reading bag_grads [B, d]
  expanded          ha_sparse_opt_fused_f32ids on a gradient expanded to [n, d] BEFORE the window (existing code)
  expand+expanded   the expansion gather (IndexedSlices.expanded_values: ha_gather_u64ids) timed inside the window as well:
                    what a pooled model pays without the bag call

Every call sorts its plan, as the one-call form does.  A window is `--iters` calls over `--distinct` different batches
(herald_amd.synth.criteo_batch), captured into one device graph so that the device runs them back to back, between two device
events; the figure of a window is its time / iters (tools/bag_bench.py's time_variants).  Every variant is warmed up before
anything is timed.  Reported per variant: median, minimum and maximum over the windows, and the bytes the algorithm needs
(computed from the shapes and the batches' unique counts, below) over the median.

The feature's condition is evaluated per shape and optimizer: bags <= expanded, where a difference within the larger of the
two variants' own window spreads counts as equal (tools/bag_bench.py's rule).

Kernel times: run under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bag_opt_bench.py --no-graph --reps 1 ...` (the
kernels are apply_opt_bags_kernel / apply_opt_kernel up to 36,864 ids, apply_listed_kernel beyond, and the plan's sort).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from bag_bench import init_table, summarise, time_variants, verdict
from herald_amd import ops, synth

STATES = {"adagrad": 1, "adam": 2}


def algorithmic_bytes(B, F, d, U, kind):
    """Per call: the ids read by the sort, sorted keys + occurrence indices written and read back, the gradient rows that are
    distinct, and every unique row of the parameter and of each state read and written once."""
    n = B * F
    plan = n * 4 + 2 * n * 8
    rows = U * 8 * d * (1 + STATES[kind])
    return {"bags": plan + B * 4 * d + rows,
            "expanded": plan + n * 4 * d + rows,
            "expand+expanded": plan + (B * 4 * d + n * 8 + n * 4 * d) + n * 4 * d + rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x26x512,4096x26x128", help="B x F x d, comma separated")
    ap.add_argument("--kinds", default="adagrad,adam")
    ap.add_argument("--rows", type=int, default=synth.CRITEO_ROWS)
    ap.add_argument("--reps", type=int, default=15, help="timed windows per variant")
    ap.add_argument("--iters", type=int, default=200, help="calls per window")
    ap.add_argument("--distinct", type=int, default=32, help="different batches cycled through a window")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--no-graph", action="store_true", help="plain launches instead of one device graph per window")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args()
    kinds = args.kinds.split(",")
    for k in kinds:
        if k not in STATES:
            raise SystemExit("--kinds: adagrad and / or adam, got %r" % k)
    if not torch.cuda.is_available():
        raise SystemExit("bag_opt_bench.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    results = {"rows": args.rows, "reps": args.reps, "iters": args.iters, "distinct": args.distinct,
               "graph": not args.no_graph, "device": torch.cuda.get_device_name(dev), "shapes": {}}
    table, s1, s2, table_d = None, None, None, None
    for (B, F, d) in shapes:
        if table_d != d:
            table = s1 = s2 = None
            torch.cuda.empty_cache()
            table, table_d = init_table(args.rows, d, dev), d
            s1, s2 = torch.zeros_like(table), torch.zeros_like(table)     # the full-size states, beside the table
        n = B * F
        host = [synth.as_f32_ids(synth.criteo_batch(B, step=s, rows=args.rows, nfields=F)) for s in range(args.distinct)]
        U = float(np.mean([np.unique(h).size for h in host]))
        ids = [torch.from_numpy(h).to(dev) for h in host]
        flat = [t.reshape(-1) for t in ids]
        nd = len(ids)
        plan = ops.IndexPlan(n, dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(456)
        bag_grads = torch.randn((B, d), dtype=torch.float32, device=dev, generator=gen)
        expanded = bag_grads.repeat_interleave(F, 0).contiguous()
        scratch = torch.empty_like(expanded)
        which = torch.arange(n, dtype=torch.int64, device=dev) // F
        entry = {"n": n, "mean_unique": U, "kinds": {}, "conditions": {}}
        print("== B=%d F=%d d=%d  n=%d  mean unique %.0f" % (B, F, d, n, U))
        for kind in kinds:
            st2 = s2 if kind == "adam" else None
            hyper = dict(lr=args.lr, eps=1e-7, beta1t=0.9 ** 3, beta2t=0.999 ** 3)

            def bags(i):
                ops.sparse_opt_fused_bags(kind, table, ids[i % nd], bag_grads, s1, st2, plan=plan, **hyper)

            def expand(i):
                ops.sparse_opt_fused(kind, table, flat[i % nd], expanded, s1, st2, plan=plan, **hyper)

            def expand_expand(i):
                ops.embedding_lookup(bag_grads, which, out=scratch)      # what IndexedSlices.expanded_values launches
                ops.sparse_opt_fused(kind, table, flat[i % nd], scratch, s1, st2, plan=plan, **hyper)

            res = summarise(time_variants({"bags": bags, "expanded": expand, "expand+expanded": expand_expand}, args.reps,
                                          args.iters, not args.no_graph, dev), algorithmic_bytes(B, F, d, U, kind))
            entry["kinds"][kind] = res
            v = entry["conditions"][kind + ": bags<=expanded"] = verdict(res, "bags", "expanded")
            for name, r in res.items():
                print("  %-8s %-16s median %8.2f us  [%7.2f .. %7.2f]  %6.2f MB  %7.1f GB/s" % (
                    kind, name, r["median_us"], r["min_us"], r["max_us"], r["bytes"] / 1e6, r["GBps_at_median"]))
            print("  condition %s bags<=expanded %s  (difference %+.2f us, spread %.2f us)" % (
                kind, "met" if v["met"] else "MISSED", v["a_minus_b_us"], v["spread_us"]))
            sys.stdout.flush()
        results["shapes"]["%dx%dx%d" % (B, F, d)] = entry
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
