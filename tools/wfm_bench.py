#!/usr/bin/env python3
"""The weighted FM-pooled step of the FAE DeepFM's second-order table (forward, backward, both), fused against composed, on the
full Criteo-sized table.

Per shape (B, F, d) and mask class -- all ones, half the occurrences dead, 85 % dead; a dead occurrence carries weight 0 and the
padding id 0 -- two candidates are timed in ONE process, alternating, `--reps` windows each, for the forward, the backward and
both together:

  (a) fused      ha_gather_wfm_f32ids; ha_sgd_sparse_update_wfm_bags_f32ids (masked keys + plan + the weighted FM apply)
  (b) composed   what such a model needs without the fused forms: ha_gather_f32ids to [n, d], then the PyTorch mask / sum /
                 square-sum passes (x = rows * w, S = sum x, Q = sum x * x); backward ha_wfm_grad_rows over the rows the forward
                 kept and ha_sgd_sparse_update_f32ids on the [n, d] gradient

Every update plans its batch inside the call, so both pay for their plan.  The dead fractions are synthetic: the ids are
herald_amd.synth.criteo_batch's, the dead occurrences are drawn uniformly; nobody has measured the reference's datasets here.
The protocol is tools/wbag_bench.py's: a window is `--iters` steps over `--distinct` different batches, captured into one device
graph so that the device runs them back to back, between two device events; the figure of a window is its time / iters.  Every
candidate is warmed up before anything is timed.  Reported per candidate: median, minimum and maximum over the windows.  There is
no threshold: where (a) is not faster than (b) outside the spread the line says so.
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
from wbag_bench import MASKS, summarise, time_variants   # noqa: E402  (the same windows)


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
        raise SystemExit("wfm_bench.py measures on the GPU; there is none here")
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
        g_s = torch.randn((B, d), dtype=torch.float32, device=dev, generator=gen) * 0.1
        g_q = torch.randn((B, d), dtype=torch.float32, device=dev, generator=gen) * 0.1
        out_s = torch.empty((B, d), dtype=torch.float32, device=dev)
        out_q = torch.empty((B, d), dtype=torch.float32, device=dev)
        rows_out = torch.empty((B, F, d), dtype=torch.float32, device=dev)
        x = torch.empty((B, F, d), dtype=torch.float32, device=dev)
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
                ops.embedding_lookup_wfm(table, ids[i % nd], ws[i % nd], sum_out=out_s, sq_out=out_q)

            def fwd_composed(i):
                ops.embedding_lookup(table, ids[i % nd], out=rows_out)
                torch.mul(rows_out, ws[i % nd].unsqueeze(-1), out=x)
                torch.sum(x, dim=1, out=out_s)
                x.mul_(x)
                torch.sum(x, dim=1, out=out_q)

            def bwd_fused(i):
                ops.sgd_sparse_update_wfm_bags(table, ids[i % nd], g_s, g_q, ws[i % nd], args.lr)

            def bwd_composed(i):
                # (rows_out: the rows the forward gathered and a model would have kept for this)
                ops.wfm_grad_rows(g_s, g_q, ws[i % nd].reshape(-1), rows_out, bag=F, out=x)
                ops.sgd_sparse_update(table, ids[i % nd].reshape(-1), x.view(n, d), args.lr)

            phases = {
                "forward": {"fused": fwd_fused, "composed": fwd_composed},
                "backward": {"fused": bwd_fused, "composed": bwd_composed},
                "both": {"fused": lambda i: (fwd_fused(i), bwd_fused(i)), "composed": lambda i: (fwd_composed(i), bwd_composed(i))},
            }
            entry = {"n": n, "dead_share": MASKS[mask], "mean_live_unique": live_u, "longest_run": longest, "phases": {}}
            print("== B=%d F=%d d=%d mask=%s  n=%d  mean live unique %.0f  longest run of one key %d"
                  % (B, F, d, mask, n, live_u, longest))
            for phase, variants in phases.items():
                res = summarise(time_variants(variants, args.reps, args.iters, not args.no_graph, dev))
                cmp = {"fused vs composed": compare(res, "fused", "composed")}
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
