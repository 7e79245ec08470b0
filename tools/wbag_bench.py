#!/usr/bin/env python3
"""The weighted sum-pooled step of an FAE model's main table (forward, backward, both), fused against composed, on the full
Criteo-sized table.

Per shape (B, F, d) and mask class -- all ones, half the occurrences dead, 85 % dead; a dead occurrence carries weight 0 and the
padding id 0 -- three candidates are timed in ONE process, alternating, `--reps` windows each, for the forward, the backward and
both together:

  (a) fused      ha_gather_wsum_f32ids; ha_sgd_sparse_update_wbags_f32ids (masked keys + plan + the weighted apply)
  (b) composed   what the operators gave before there were weights: ha_gather_f32ids to [n, d], a multiply over [n, d] and a
                 sum; the pooled gradient expanded to [n, d] (the gather kernel over it), a multiply, ha_sgd_sparse_update_f32ids
  (c) bound      the unweighted ha_gather_sum_f32ids / ha_sgd_sparse_update_bags_f32ids on the same ids: they move the same
                 rows without weights (and walk the padding id's run) -- the bound for (a), not a variant of the step

Every update plans its batch inside the call, so all three pay for their plan.  The dead fractions are synthetic: the ids are
herald_amd.synth.criteo_batch's, the dead occurrences are drawn uniformly; nobody has measured the reference's datasets here.
A window is `--iters` steps over `--distinct` different batches, captured into one device graph so that the device runs them
back to back, between two device events; the figure of a window is its time / iters.  Every candidate is warmed up before
anything is timed.  Reported per candidate: median, minimum and maximum over the windows.  There is no threshold: where (a) is
not faster than (b) outside the spread the line says so.
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
from bag_bench import init_table                     # noqa: E402  (the same table)
from fm_bench import compare                         # noqa: E402

MASKS = {"ones": 0.0, "half": 0.5, "dead85": 0.85}      # share of dead occurrences


def time_variants(variants, reps, iters, use_graph, dev):
    """bag_bench.time_variants on ONE side stream for warm-up, capture and replay: the one-call updates keep their plan in a
    per-stream scratch that grows on demand, and nothing may be allocated while a graph is captured -- so the warm-up has to
    have run on the stream that is captured.  variants: {name: f(i)}; -> {name: [microseconds per call, one per window]}."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    runs = {}
    with torch.cuda.stream(side):
        for name, f in variants.items():
            for i in range(min(iters, 8)):                  # warm-up: code objects, allocator, the scratch
                f(i)
            side.synchronize()
            if use_graph:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    for i in range(iters):
                        f(i)
                runs[name] = g.replay
                g.replay()                                  # warm-up of the graph itself
            else:
                runs[name] = (lambda f=f: [f(i) for i in range(iters)])
        side.synchronize()
        times = {name: [] for name in variants}
        for _ in range(reps):
            for name, run in runs.items():                  # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                times[name].append(1e3 * e0.elapsed_time(e1) / iters)
    torch.cuda.current_stream(dev).wait_stream(side)
    return times


def summarise(times):
    return {name: {"median_us": float(np.median(ts)), "min_us": float(min(ts)), "max_us": float(max(ts)), "windows": len(ts)}
            for name, ts in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x26x128,256x26x512,4096x26x128", help="B x F x d, comma separated")
    ap.add_argument("--masks", default="ones,half,dead85", help="mask classes, comma separated: " + ", ".join(MASKS))
    ap.add_argument("--rows", type=int, default=synth.CRITEO_ROWS)
    ap.add_argument("--reps", type=int, default=15, help="timed windows per candidate")
    ap.add_argument("--iters", type=int, default=200, help="steps per window")
    ap.add_argument("--distinct", type=int, default=32, help="different batches cycled through a window")
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--no-graph", action="store_true", help="plain launches instead of one device graph per window")
    ap.add_argument("--out", default=None, help="write the results as JSON here")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wbag_bench.py measures on the GPU; there is none here")
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
        raw = [synth.as_f32_ids(synth.criteo_batch(B, step=s, rows=args.rows, nfields=F)) for s in range(args.distinct)]
        gen = torch.Generator(device=dev)
        gen.manual_seed(456)
        g = torch.randn((B, d), dtype=torch.float32, device=dev, generator=gen) * 0.1
        out = torch.empty((B, d), dtype=torch.float32, device=dev)
        rows_out = torch.empty((B, F, d), dtype=torch.float32, device=dev)
        g_rows = torch.empty((B, F, d), dtype=torch.float32, device=dev)
        which = torch.arange(n, dtype=torch.int64, device=dev) // F
        for mask in args.masks.split(","):
            rng = np.random.default_rng(789)
            host_w = [(rng.random(h.shape) >= MASKS[mask]).astype(np.float32) for h in raw]
            host = [np.where(w != 0, h, np.float32(0)) for h, w in zip(raw, host_w)]
            longest = int(max(np.unique(h, return_counts=True)[1].max() for h in host))
            live_u = float(np.mean([np.unique(h[w != 0]).size for h, w in zip(host, host_w)]))
            ids = [torch.from_numpy(h).to(dev) for h in host]
            ws = [torch.from_numpy(w).to(dev) for w in host_w]
            nd = len(ids)
            torch.cuda.synchronize(dev)

            def fwd_fused(i):
                ops.embedding_lookup_wsum(table, ids[i % nd], ws[i % nd], out=out)

            def fwd_composed(i):
                ops.embedding_lookup(table, ids[i % nd], out=rows_out)
                torch.sum(rows_out * ws[i % nd].unsqueeze(-1), dim=1, out=out)

            def fwd_bound(i):
                ops.embedding_lookup_sum(table, ids[i % nd], out=out)

            def bwd_fused(i):
                ops.sgd_sparse_update_wbags(table, ids[i % nd], g, ws[i % nd], args.lr)

            def bwd_composed(i):
                ops.embedding_lookup(g, which, out=g_rows)
                g_rows.mul_(ws[i % nd].unsqueeze(-1))
                ops.sgd_sparse_update(table, ids[i % nd].reshape(-1), g_rows.view(n, d), args.lr)

            def bwd_bound(i):
                ops.sgd_sparse_update_bags(table, ids[i % nd], g, args.lr)

            phases = {
                "forward": {"fused": fwd_fused, "composed": fwd_composed, "bound": fwd_bound},
                "backward": {"fused": bwd_fused, "composed": bwd_composed, "bound": bwd_bound},
                "both": {"fused": lambda i: (fwd_fused(i), bwd_fused(i)), "composed": lambda i: (fwd_composed(i), bwd_composed(i)),
                         "bound": lambda i: (fwd_bound(i), bwd_bound(i))},
            }
            entry = {"n": n, "dead_share": MASKS[mask], "mean_live_unique": live_u, "longest_run": longest, "phases": {}}
            print("== B=%d F=%d d=%d mask=%s  n=%d  mean live unique %.0f  longest run of one key %d"
                  % (B, F, d, mask, n, live_u, longest))
            for phase, variants in phases.items():
                res = summarise(time_variants(variants, args.reps, args.iters, not args.no_graph, dev))
                cmp = {"fused vs composed": compare(res, "fused", "composed"), "fused vs bound": compare(res, "fused", "bound")}
                entry["phases"][phase] = {"variants": res, "comparisons": cmp}
                for name, r in res.items():
                    print("  %-8s %-9s median %8.2f us  [%7.2f .. %7.2f]  over %d windows"
                          % (phase, name, r["median_us"], r["min_us"], r["max_us"], r["windows"]))
                for name, v in cmp.items():
                    print("  %-8s %-18s %s is %s  (difference %+.2f us, spread %.2f us)"
                          % (phase, name, v["a"], v["a_is"], v["a_minus_b_us"], v["spread_us"]))
                sys.stdout.flush()
            results["shapes"]["%dx%dx%d/%s" % (B, F, d, mask)] = entry
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
